"""`lash dist --derep D`: the arguments are checked before any file is read or any device is touched, so no GPU is needed here."""
import os
import subprocess

import pytest

import host_lib as H


def _dist(tmp_path, *extra):
    if not os.path.exists(H.CLI):
        pytest.skip("the lash command line has not been built")
    return subprocess.run([H.CLI, "dist", "-q", "none", "-r", "none", "-o", "out.tsv"] + list(extra), cwd=tmp_path, capture_output=True, text=True,
                          timeout=60)


@pytest.mark.parametrize("value", ["abc", "inf", "-inf", "nan", "", "0.05x"])
def test_derep_must_be_a_finite_number(tmp_path, value):
    r = _dist(tmp_path, "--derep", value)
    assert r.returncode == 2 and "--derep" in r.stderr
    assert not (tmp_path / "out.tsv").exists()


@pytest.mark.parametrize("other", [["--dm"], ["--top", "3"], ["--max-dist", "0.1"], ["--cluster", "0.05"]])
def test_derep_with_another_output_form_is_refused(tmp_path, other):
    for args in (["--derep", "0.05"] + other, other + ["--derep", "0.05"]):
        r = _dist(tmp_path, *args)
        assert r.returncode == 2 and "--derep" in r.stderr and other[0] in r.stderr
        assert not (tmp_path / "out.tsv").exists()


def test_derep_on_more_than_one_worker_is_refused(tmp_path):
    for args in (["--derep", "0.05", "--devices", "0,0"], ["--devices", "0,1", "--derep", "0.05"]):
        r = _dist(tmp_path, *args)
        assert r.returncode == 2 and "--derep" in r.stderr and "--devices" in r.stderr and "row order" in r.stderr
        assert not (tmp_path / "out.tsv").exists()


@pytest.mark.parametrize("value", ["0.05", "0", "1", "-0.25", "1e-3", "7"])
def test_a_valid_derep_is_accepted(tmp_path, value):
    # accepted: the run goes on and fails at the missing sketch files, as it would without the option
    want = _dist(tmp_path)
    for extra in ([], ["--devices", "0"], ["--file-order", "-t", "4", "--block-rows", "7"]):
        r = _dist(tmp_path, "--derep", value, *extra)
        assert r.returncode == want.returncode == 1 and r.stderr == want.stderr
        assert not (tmp_path / "out.tsv").exists()


def test_help_names_derep():
    if not os.path.exists(H.CLI):
        pytest.skip("the lash command line has not been built")
    r = subprocess.run([H.CLI, "--help"], capture_output=True, text=True, timeout=60)
    text = r.stdout + r.stderr
    assert "--derep <D>" in text and "Representative" in text
    at = text.index("--derep <D>")
    assert "--file-order" in text[at:at + 700]                            # how a user sets the priority
