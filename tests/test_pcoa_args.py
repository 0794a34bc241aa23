"""`lash dist --pcoa K`: the arguments are checked before any file is read or any device is touched, so no GPU is needed here."""
import os
import subprocess

import pytest

import host_lib as H


def _dist(tmp_path, *extra, q="none", r="none"):
    assert os.path.exists(H.CLI), "the lash command line has not been built"
    return subprocess.run([H.CLI, "dist", "-q", q, "-r", r, "-o", "out.tsv"] + list(extra), cwd=tmp_path, capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("value", ["0", "17", "2.5", "x", "", "-1"])
def test_k_must_be_an_integer_from_1_to_16(tmp_path, value):
    r = _dist(tmp_path, "--pcoa", value)
    assert r.returncode == 2 and "--pcoa" in r.stderr and "1 to 16" in r.stderr
    assert not (tmp_path / "out.tsv").exists()


@pytest.mark.parametrize("other", [["--dm"], ["--top", "3"], ["--max-dist", "0.1"], ["--cluster", "0.05"], ["--derep", "0.05"], ["--containment", "query"],
                                   ["--tree"], ["--tree", "--nj"], ["--cluster", "0.05", "--linkage", "average"]])
def test_pcoa_with_another_output_form_is_refused(tmp_path, other):
    for args in (["--pcoa", "3"] + other, other + ["--pcoa", "3"]):
        r = _dist(tmp_path, *args)
        assert r.returncode == 2 and "--pcoa cannot be used with " + other[0] in r.stderr, r.stderr
        assert not (tmp_path / "out.tsv").exists()


def test_each_refusal_has_its_own_message(tmp_path):
    seen = set()
    for other in (["--dm"], ["--top", "3"], ["--max-dist", "0.1"], ["--cluster", "0.05"], ["--derep", "0.05"], ["--containment", "query"], ["--tree"]):
        seen.add(_dist(tmp_path, "--pcoa", "3", *other).stderr)
    assert len(seen) == 7
    r = _dist(tmp_path, "--pcoa", "3", "--tree", "--nj")
    assert r.returncode == 2 and "--pcoa" in r.stderr
    r = _dist(tmp_path, "--pcoa", "3", "--linkage", "single")
    assert r.returncode == 2 and "--linkage" in r.stderr


def test_pcoa_is_all_vs_all_only(tmp_path):
    r = _dist(tmp_path, "--pcoa", "3", q="a", r="b")
    assert r.returncode == 2 and "--pcoa needs an all-vs-all run" in r.stderr


@pytest.mark.parametrize("value", ["1", "3", "16"])
def test_a_valid_k_is_accepted(tmp_path, value):
    # accepted: the run goes on and fails at the missing sketch files, as it would without the option
    r = _dist(tmp_path, "--pcoa", value)
    want = _dist(tmp_path)
    assert r.returncode == want.returncode == 1 and r.stderr == want.stderr
    assert not (tmp_path / "out.tsv").exists()


def test_help_names_pcoa():
    assert os.path.exists(H.CLI), "the lash command line has not been built"
    r = subprocess.run([H.CLI, "--help"], capture_output=True, text=True, timeout=60)
    text = r.stdout + r.stderr
    assert "--pcoa <K>" in text and "#Eigenvalue" in text and "#Explained" in text
