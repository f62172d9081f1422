"""What a context knows about its bound noise textures, and the steps that keep it consistent across a rebind: NoiseHeld and the derived values of
csrc/noise_set.h, compiled with g++ (tests/noise_set_host/noise_set_host.cpp: the header includes nothing of HIP) and walked against a model written
from the library's rules.

  step                          answer                                  effect
    request_exact (mode)          -                                       remembered; nothing else changes until the next bound
    begin_rebind                  -                                       nothing is had
    bound (inexact, range, lod5)  cell32: inexact != 0 or requested       the three values and cell32 are recorded; had or not stays as it was
    ready                         -                                       the set is had
    rejects (coverage, window)    window off: -1, 2, 0                    none that a caller can see: the answer is a function of the LAST bound range
                                  on: height_window(coverage, range / 255),   and the arguments, whatever was asked before (the cache inside is one
                                  ct_mode 1 if rmin >= 128, 2 if rmax <= 127   entry per coverage value and is emptied by begin_rebind and bound)

The height windows the model expects are bake.h's own, printed by the same program from a direct call: nothing of height_window is restated here.
Nothing here touches a GPU."""
import itertools
import os
import struct
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "tests", "noise_set_host")


def bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


SHIPPED = (151, 231, 255)        # min R, max R, max B of the shipped weather.bmp: what the host tools' own scans gave before they shared weather_range
STRATUS = (75, 115, 200)         # every cloud type <= 127, another max B: another window and ct_mode 2
UNBOUND = (0, 255, 255)          # what a context that has never bound a set holds
COVERAGES = (bits(0.2), bits(0.35))
LOD5 = bits(0.4375)
OFF = (bits(-1.0), bits(2.0), 0)

# the alphabet of the walk: (name, argument, command line)
STEPS = (("request_exact", 0, "request_exact 0"), ("request_exact", 1, "request_exact 1"), ("begin_rebind", None, "begin_rebind"), ("ready", None, "ready")) + \
    tuple(("bound", (n, r), "bound %d %d %d %d %d" % ((n,) + r + (LOD5,))) for n, r in ((0, SHIPPED), (7, SHIPPED), (0, STRATUS))) + \
    tuple(("rejects", (c, w), "rejects %d %d" % (c, w)) for c in COVERAGES for w in (1, 0))

FRESH = dict(have=False, cell32=False, inexact=0, lod5=0)


def ct_mode(r):
    return 1 if r[0] >= 128 else (2 if r[1] <= 127 else 0)


def run(text_in):
    r = subprocess.run([os.path.join(DIR, "noise_set_host")], input=text_in, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0, r.stdout[-2000:]
    return [tuple(int(x) for x in ln.split()) for ln in r.stdout.splitlines()]


@pytest.fixture(scope="module")
def tool():
    subprocess.check_call(["make", "-C", DIR, "-s"])
    return run


@pytest.fixture(scope="module")
def windows(tool):
    """(coverage, range) -> (lo, hi) of a direct call of bake.h height_window"""
    keys = [(c, r) for c in COVERAGES for r in (SHIPPED, STRATUS, UNBOUND)]
    out = tool("".join("window %d %d %d %d\n" % ((c,) + r) for c, r in keys))
    w = dict(zip(keys, out))
    assert len(set(w.values())) == len(keys), w              # six different windows: an answer for another coverage or range cannot pass for the right one
    return w


def parse(v):
    assert len(v) == 8, v
    return dict(have=bool(v[0]), cell32=bool(v[1]), inexact=v[2], lod5=v[3]), v[4], tuple(v[5:8])


def test_every_walk_of_up_to_four_steps_matches_the_model(tool, windows):
    """11 + 121 + 1331 + 14641 sequences over the eleven steps from a fresh state: the answer of every step and the state after it."""
    seqs = [seq for n in range(1, 5) for seq in itertools.product(range(len(STEPS)), repeat=n)]
    assert len(STEPS) == 11 and len(seqs) == 16104
    # (an uncached rejects is some milliseconds of bisection in height_window: eight processes, each a share of the sequences)
    with ThreadPoolExecutor(8) as pool:
        shares = pool.map(lambda k: tool("".join("reset\n" + "".join(STEPS[t][2] + "\n" for t in seq) for seq in seqs[k::8])), range(8))
        lines = [ln for k, share in enumerate(shares) for ln in share]
    seqs = [seq for k in range(8) for seq in seqs[k::8]]
    assert len(lines) == sum(1 + len(seq) for seq in seqs)
    at = 0
    same_coverage_other_range = late_requests = unready = 0
    for seq in seqs:
        got = parse(lines[at]); at += 1
        assert got == (FRESH, 0, (0, 0, 0)), seq
        s, requested, rng, rebinding = dict(FRESH), False, UNBOUND, False
        asked = {}                                           # coverage -> the range it was last asked for with the window on
        for i, t in enumerate(seq):
            name, arg, _ = STEPS[t]
            before = dict(s)
            answer, rej = 0, (0, 0, 0)
            if name == "request_exact":
                requested = arg == 1
                late_requests += s["cell32"] != requested
            elif name == "begin_rebind":
                s["have"] = False; rebinding = True
            elif name == "bound":
                s["inexact"], rng = arg
                s["lod5"] = LOD5
                s["cell32"] = s["inexact"] != 0 or requested
                answer = int(s["cell32"])
            elif name == "ready":
                s["have"] = True; rebinding = False
            else:
                cov, win = arg
                rej = windows[(cov, rng)] + (ct_mode(rng),) if win else OFF
                if win:
                    same_coverage_other_range += asked.get(cov, rng) != rng
                    asked[cov] = rng
            got = parse(lines[at]); at += 1
            where = ([STEPS[k][2] for k in seq], i)
            assert got == (s, answer, rej), (where, got, (s, answer, rej))
            if name == "request_exact":
                assert got[0] == before, where               # a request changes nothing until the next bound
            if rebinding:
                assert not got[0]["have"], where             # nothing is had between begin_rebind and ready
                unready += 1
    assert at == len(lines)
    assert same_coverage_other_range > 0 and late_requests > 0 and unready > 0     # the walk reaches each of the three


def test_a_rebind_to_another_range_answers_with_the_new_window_at_the_same_coverage(tool, windows):
    cov = COVERAGES[0]
    bind = lambda r: ["begin_rebind", "bound 0 %d %d %d %d" % (r + (LOD5,)), "ready"]
    ask = "rejects %d 1" % cov
    out = tool("\n".join(["reset"] + bind(SHIPPED) + [ask, ask] + bind(STRATUS) + [ask] + bind(SHIPPED) + [ask]) + "\n")
    got = [parse(v)[2] for v in out]
    assert got[4] == got[5] == got[13] == windows[(cov, SHIPPED)] + (1,)
    assert got[9] == windows[(cov, STRATUS)] + (2,) and got[9] != got[4]


def test_a_nan_coverage_is_answered_like_a_direct_call(tool):
    nan = bits(float("nan"))
    out = tool("reset\nbound 0 %d %d %d %d\nrejects %d 1\nrejects %d 1\nwindow %d %d %d %d\n" % (SHIPPED + (LOD5, nan, nan, nan) + SHIPPED))
    assert parse(out[2])[2] == parse(out[3])[2] == out[4] + (1,) == OFF[:2] + (1,)


def test_the_integer_and_the_double_ct_mode_rules_agree_on_every_range(tool):
    """noise_set.h decides ct_mode on texel values (rmin >= 128, rmax <= 127), as the host tools always did; the library used to decide it on the doubles
    it had divided by 255 (x / 255.0 * 255.0 >= 127.5, <= 127.5; Python's floats are the same IEEE doubles).  All 256 x 256 (rmin, rmax) pairs,
    inconsistent ones (rmin > rmax) included."""
    out = tool("ctmodes\n")
    assert len(out) == 65536
    for k, (got,) in enumerate(out):
        r = (k >> 8, k & 255, 255)
        dmin, dmax = r[0] / 255.0, r[1] / 255.0
        double = 1 if dmin * 255.0 >= 127.5 else (2 if dmax * 255.0 <= 127.5 else 0)
        assert got == double == ct_mode(r), r
    assert {v[0] for v in out} == {0, 1, 2}


def test_the_weather_range_of_the_shipped_map(tool, tmp_path):
    import gvcd_amd
    weather = gvcd_amd.assets.load_default_noise()[2]
    assert weather.shape == (512, 512, 3) and weather.dtype == np.uint8
    path = tmp_path / "weather.rgb8"
    path.write_bytes(np.ascontiguousarray(weather).tobytes())
    assert tool("weather_range %s\n" % path) == [SHIPPED]
    w2 = weather.copy(); w2[..., 0] //= 2; w2[..., 2] = np.minimum(w2[..., 2], 200); w2[511, 511, 0] = 1
    path.write_bytes(w2.tobytes())
    assert tool("weather_range %s\n" % path) == [(1, 115, 200)]


def test_the_detail_lod5_texel(tool):
    """hfbm = (5 r + 2 g + b) / (8 * 255) of clouds.glsl:133, in fp32 as the kernels' other taps deliver it"""
    texels = [(0, 0, 0), (255, 255, 255), (10, 20, 30), (255, 0, 0), (0, 255, 0), (0, 0, 255), (131, 7, 64)]
    out = tool("".join("lod5 %d %d %d\n" % t for t in texels))
    for (r, g, b), (got,) in zip(texels, out):
        want = np.float32(5 * r + 2 * g + b) * (np.float32(1.0) / (np.float32(8.0) * np.float32(255.0)))
        assert got == bits(float(want)), (r, g, b)
