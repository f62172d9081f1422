"""W7: the host generator of the weather map and its parameter check under the address and undefined-behaviour sanitizers, in a stand-alone program
of its own (tests/weather_asan: its own main, built with -fsanitize=address,undefined), run here on the CPU.  The program is not loaded into Python
and nothing of it runs on a GPU."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "tests", "weather_asan")


def fnv(a):
    h = 2166136261
    for b in a.tobytes():
        h = ((h ^ b) * 16777619) & 0xFFFFFFFF
    return h


def test_w7_the_generator_and_its_check_run_clean_under_the_sanitizers(pkg):
    subprocess.check_call(["make", "-C", DIR, "-s"])
    r = subprocess.run([os.path.join(DIR, "weather_asan")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    words = r.stdout.split()
    assert words[:3] == ["weather", "asan", "ok"]
    assert int(words[3], 16) == fnv(pkg.assets.generate_weather(1))   # the sanitized build generates the library's bytes
