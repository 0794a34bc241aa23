"""`lash dist --top K`: the arguments are checked before any file is read or any device is touched, so no GPU is needed here."""
import os
import subprocess

import pytest

import host_lib as H


def _dist(tmp_path, *extra):
    if not os.path.exists(H.CLI):
        pytest.skip("the lash command line has not been built")
    return subprocess.run([H.CLI, "dist", "-q", "none", "-r", "none"] + list(extra), cwd=tmp_path, capture_output=True, text=True, timeout=60)


def test_top_with_dm_is_refused(tmp_path):
    r = _dist(tmp_path, "--top", "5", "--dm")
    assert r.returncode == 2 and "--top" in r.stderr and "--dm" in r.stderr


@pytest.mark.parametrize("value", ["0", "-1", "1.5", "abc", "1025", "", "5x", "99999999999999999999999"])
def test_top_must_be_an_integer_from_1_to_1024(tmp_path, value):
    r = _dist(tmp_path, "--top", value)
    assert r.returncode == 2 and "--top" in r.stderr


@pytest.mark.parametrize("extra", [["--top", "1"], ["--top", "10"], ["--top", "1024"], ["--top", "3", "--max-dist", "0.05"]])
def test_a_valid_top_is_accepted(tmp_path, extra):
    # accepted: the run goes on and fails at the missing sketch files, as it would without the option
    r = _dist(tmp_path, *extra)
    want = _dist(tmp_path)
    assert r.returncode == want.returncode == 1 and r.stderr == want.stderr


def test_help_names_top():
    if not os.path.exists(H.CLI):
        pytest.skip("the lash command line has not been built")
    r = subprocess.run([H.CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert "--top <K>" in r.stdout + r.stderr
