"""The streaming step-response accumulator of the evaluation kernel (b747_rl_ctrl_amd/csrc/b747_stepinfo.h, fed one
sample at a time through tests/native/stepinfo_check.cpp) against the restated calc_stepinfo (oracle/stepinfo_ref.py,
tools/general.py:46-61) over the whole series: exact (the same float64 expressions), None <-> NaN.  Series: the six
of tests/test_stepinfo.py and 16 random damped responses of both signs, each whole, cut at a random length, and cut to
one and two samples (the rise test excludes the last sample, so these are its edge cases)."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

from stepinfo_ref import calc_stepinfo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("overshoot", "rise_time", "settling_time", "static_error")


@pytest.fixture(scope="module")
def stream(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("stepinfo") / "libstepinfo_check.so")
    subprocess.run(["g++", "-O2", "-fPIC", "-shared", "-std=c++17", "-ffp-contract=off", "-o", so,
                    os.path.join(ROOT, "tests", "native", "stepinfo_check.cpp")], check=True)
    L = ctypes.CDLL(so)
    P = ctypes.POINTER(ctypes.c_double)
    L.stepinfo_stream.argtypes = [P, P, ctypes.c_int, ctypes.c_double, ctypes.c_double, P]
    L.stepinfo_stream.restype = None

    def run(ys, ts, y_base, band=0.05):
        ys, ts = np.ascontiguousarray(ys, np.float64), np.ascontiguousarray(ts, np.float64)
        out = np.zeros(4)
        L.stepinfo_stream(ys.ctypes.data_as(P), ts.ctypes.data_as(P), len(ys), float(y_base), band, out.ctypes.data_as(P))
        return dict(zip(KEYS, out))
    return run


def _series():
    t = np.arange(1, 401) * 0.01
    yield "overshooting", 5 * (1 - np.exp(-t / 0.3) * np.cos(8 * t)), 5.0, t
    yield "negative_ref", -3 * (1 - np.exp(-t / 0.5)), -3.0, t
    yield "never_rises", 0.5 * (1 - np.exp(-t)), 4.0, t
    yield "settled_from_start", 2.0 + 0 * t, 2.0 + 1e-9, t
    yield "zero_ref", np.sin(t), 0.0, t
    yield "ramp_inside_band_at_end", np.linspace(0, 1.0, 400), 1.0, t
    rng = np.random.default_rng(0)
    t = np.arange(1, 301) * 0.05
    for j in range(16):
        b = rng.uniform(1, 10) * rng.choice([-1, 1])
        tau, w = rng.uniform(0.1, 3), rng.uniform(1, 8)
        ys = b * (1 - np.exp(-t / tau)) + 0.3 * b * np.exp(-t / (2 * tau)) * np.sin(w * t)
        yield f"damped_{j}", ys, float(ys[-1] * (1 + rng.uniform(-0.01, 0.01))), t


def _cases():
    rng = np.random.default_rng(1)
    for name, ys, yb, ts in _series():
        cut = int(rng.integers(3, len(ys)))
        for tag, n in (("whole", len(ys)), (f"cut{cut}", cut), ("len1", 1), ("len2", 2)):
            yield f"{name}-{tag}", ys[:n], yb, ts[:n]


@pytest.mark.parametrize("name,ys,yb,ts", list(_cases()), ids=[c[0] for c in _cases()])
def test_streaming_accumulator_equals_calc_stepinfo(stream, name, ys, yb, ts):
    try:
        ref = calc_stepinfo([float(y) for y in ys], float(yb), ts=[float(t) for t in ts])
    except ZeroDivisionError:
        pytest.skip("the reference raises for y_base == ys[0]")
    got = stream(ys, ts, yb)
    for k in KEYS:
        if ref[k] is None:
            assert math.isnan(got[k]), f"{name} {k}: {got[k]} vs None"
        else:
            assert got[k] == ref[k], f"{name} {k}: {got[k]!r} vs {ref[k]!r}"


def test_error_band_is_an_argument(stream):
    t = np.arange(1, 401) * 0.01
    ys = 5 * (1 - np.exp(-t / 0.3) * np.cos(8 * t))
    for band in (0.02, 0.1):
        ref = calc_stepinfo([float(y) for y in ys], 5.0, error_band=band, ts=[float(x) for x in t])
        got = stream(ys, t, 5.0, band)
        assert all(got[k] == ref[k] for k in KEYS), (band, got, ref)
