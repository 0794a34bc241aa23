"""`lash dist --containment query|reference`: what the command line refuses before any file is read or any device is touched, and the
rule itself through the host-only entry lash_dist_rows_measure on made-up pair statistics, against its restatement below.  No GPU."""
import math
import os
import subprocess

import numpy as np
import pytest

import host_lib as H


def _cli(*args, cwd=None):
    assert os.path.exists(H.CLI), "the lash command line has not been built (build() makes it)"
    return subprocess.run([H.CLI] + list(args), cwd=cwd, capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("direction", ["query", "reference"])
@pytest.mark.parametrize("other", [["--dm"], ["--cluster", "0.05"], ["--derep", "0.05"]])
def test_symmetric_routes_are_refused_by_name(tmp_path, direction, other):
    for args in (["--containment", direction] + other, other + ["--containment", direction]):
        r = _cli("dist", "-q", "none", "-r", "none", *args, cwd=tmp_path)
        assert r.returncode == 2, r.stderr
        assert "--containment" in r.stderr and other[0] in r.stderr
        assert os.listdir(tmp_path) == []


@pytest.mark.parametrize("value", ["", "both", "Query", "jaccard", "1"])
def test_unknown_value_is_refused(tmp_path, value):
    r = _cli("dist", "-q", "none", "-r", "none", "--containment", value, cwd=tmp_path)
    assert r.returncode == 2, r.stderr
    assert "--containment" in r.stderr and "query or reference" in r.stderr
    assert os.listdir(tmp_path) == []


def test_missing_value_is_refused(tmp_path):
    r = _cli("dist", "-q", "none", "-r", "none", "--containment", cwd=tmp_path)
    assert r.returncode == 2 and "--containment" in r.stderr


@pytest.mark.parametrize("extra", [[], ["--max-dist", "0.1"], ["--top", "3"], ["--top", "3", "--max-dist", "0.1", "--fp32", "-m", "0"]])
def test_rectangular_routes_are_accepted(tmp_path, extra):
    # accepted: the run goes on and fails at the missing sketch files, as it would without the flag
    r = _cli("dist", "-q", "none", "-r", "none", "--containment", "query", *extra, cwd=tmp_path)
    want = _cli("dist", "-q", "none", "-r", "none", *extra, cwd=tmp_path)
    assert r.returncode == want.returncode == 1 and r.stderr == want.stderr


def test_help_names_containment():
    r = _cli("--help")
    assert "--containment" in r.stdout + r.stderr


# ---- the rule (lash_amd/csrc/dist_pair.h), restated -------------------------------------------------------------------------------------

def _restated(sim, a_r, a_q, k, model, direction):
    """s <= 0 -> 1; frac_c = (s / (1 + s)) * ((a_r + a_q) / den), den = a_q (query) or a_r (reference); frac_c >= 1 -> +0; else the
    model's distance of frac_c"""
    if sim <= 0.0:
        return 1.0
    frac = (sim / (1.0 + sim)) * ((a_r + a_q) / (a_q if direction == "query" else a_r))
    if frac >= 1.0:
        return 0.0
    return min(-math.log(frac) / k, 1.0) if model == 1 else 1.0 - frac ** (1.0 / k)


def test_rule_on_made_up_union_estimates():
    """ull statistics are the union estimates themselves, so the similarity (a_r + a_q - u) / u is ours to choose: nested (frac_c >= 1:
    +0, never -0 or a negative distance), partial, disjoint (s <= 0: exactly 1 whatever the cardinalities, a zero one included)"""
    from lash_amd.sketch import dist_rows
    a_r = np.array([160000.0, 40000.0, 1000.0, 0.0])
    a_q = np.array([40000.0, 160000.0, 52000.0, 40000.0, 0.0])
    inter = np.array([[40000.0, 90000.0, 52000.0, 39999.0, 0.0],
                      [40000.0, 100.0, 30000.0, 40000.5, 0.0],
                      [1000.0, 0.0, 999.0, -3.0, 0.0],
                      [0.0, 0.0, 0.0, 0.0, 0.0]])
    union = a_r[:, None] + a_q[None, :] - inter
    union[3, 4] = 1.0                                                      # (0 + 0 - 1) / 1 < 0: clamped, d = 1
    for model in (0, 1):
        for direction in ("query", "reference"):
            d = dist_rows("ull", 12, 16, model, a_r, a_q, sum_or_union=union, containment=direction)
            d32 = dist_rows("ull", 12, 16, model, a_r, a_q, sum_or_union=union, containment=direction, fp32=True)
            for i in range(4):
                for j in range(5):
                    sim = (a_r[i] + a_q[j] - union[i, j]) / union[i, j]
                    want = _restated(sim, a_r[i], a_q[j], 16, model, direction)
                    assert d[i, j] == pytest.approx(want, abs=1e-15), (model, direction, i, j)
                    assert abs(d32[i, j] - want) <= 2e-6
                    if want in (0.0, 1.0):
                        assert d[i, j] == want and d32[i, j] == want and not math.copysign(1.0, d[i, j]) < 0 and not math.copysign(1.0, d32[i, j]) < 0
            assert (d[0, 0] == 0.0) == (direction == "query") and d[1, 0] == 0.0 and d[2, 1] == 1.0 and d[3, 0] == 1.0 and np.all(d >= 0.0) and np.all(d32 >= 0.0)
    # nested: all of the 40 000 query k-mers are in the reference, which is four times as large
    dq = dist_rows("ull", 12, 16, 1, a_r[:1], a_q[:1], sum_or_union=union[:1, :1], containment="query")[0, 0]
    dr = dist_rows("ull", 12, 16, 1, a_r[:1], a_q[:1], sum_or_union=union[:1, :1], containment="reference")[0, 0]
    dj = dist_rows("ull", 12, 16, 1, a_r[:1], a_q[:1], sum_or_union=union[:1, :1])[0, 0]
    assert dq == 0.0 and dr == pytest.approx(-math.log(0.25) / 16, rel=1e-12) and dj == pytest.approx(-math.log(0.4) / 16, rel=1e-12)


def test_equal_cardinalities_reduce_to_the_default_bit_for_bit():
    from lash_amd.sketch import dist_rows
    rng = np.random.default_rng(5)
    a = rng.uniform(1e3, 1e7, 64)
    sim = rng.uniform(1e-6, 1.0, 64)
    sim[:4] = (1.0, 0.5, 1e-300, 0.999999999)
    for model in (0, 1):
        for fp32 in (False, True):
            for i in range(64):
                u = np.array([[2.0 * a[i] / (1.0 + sim[i])]])             # some similarity near sim[i]: whatever it rounds to
                want = dist_rows("ull", 12, 21, model, a[i:i + 1], a[i:i + 1], sum_or_union=u, fp32=fp32)
                for direction in ("query", "reference"):
                    got = dist_rows("ull", 12, 21, model, a[i:i + 1], a[i:i + 1], sum_or_union=u, fp32=fp32, containment=direction)
                    assert got[0, 0] == want[0, 0], (model, fp32, i, direction)


def test_bad_measure_is_einval():
    import ctypes as C
    from lash_amd import _lib
    lib = _lib.load()
    one = np.ones(1)
    out = np.zeros(1)
    bad = C.c_uint64()
    for measure, rc in ((0, _lib.OK), (1, _lib.OK), (2, _lib.OK), (3, _lib.EINVAL), (-1, _lib.EINVAL)):
        assert lib.lash_dist_rows_measure(_lib.ULL, 12, 16, 1, 0, 1, 1, one.ctypes.data, one.ctypes.data, None, None, one.ctypes.data, None, None,
                                          measure, out.ctypes.data, C.byref(bad)) == rc
