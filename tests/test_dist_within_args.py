"""`lash dist --max-dist`: the arguments are checked before any file is read or any device is touched, so no GPU is needed here."""
import os
import subprocess

import pytest

import host_lib as H


def _dist(tmp_path, *extra):
    if not os.path.exists(H.CLI):
        pytest.skip("the lash command line has not been built")
    return subprocess.run([H.CLI, "dist", "-q", "none", "-r", "none"] + list(extra), cwd=tmp_path, capture_output=True, text=True, timeout=60)


def test_max_dist_with_dm_is_refused(tmp_path):
    r = _dist(tmp_path, "--max-dist", "0.05", "--dm")
    assert r.returncode == 2 and "--max-dist" in r.stderr and "--dm" in r.stderr


@pytest.mark.parametrize("value", ["abc", "nan", "NaN", "inf", "-inf", "0.1x", ""])
def test_max_dist_must_be_a_finite_number(tmp_path, value):
    r = _dist(tmp_path, "--max-dist", value)
    assert r.returncode == 2 and "--max-dist" in r.stderr


@pytest.mark.parametrize("value", ["0", "0.05", "1", "-0.5", "1e-3"])
def test_a_finite_max_dist_is_accepted(tmp_path, value):
    # accepted: the run goes on and fails at the missing sketch files, as it would without the option
    r = _dist(tmp_path, "--max-dist", value)
    want = _dist(tmp_path)
    assert r.returncode == want.returncode == 1 and r.stderr == want.stderr
