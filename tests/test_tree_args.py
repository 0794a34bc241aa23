"""`lash dist --tree` / `--linkage`: the arguments are checked before any file is read or any device is touched, so no GPU is needed here."""
import os
import subprocess

import pytest

import host_lib as H


def _dist(tmp_path, *extra, q="none", r="none"):
    if not os.path.exists(H.CLI):
        pytest.skip("the lash command line has not been built")
    return subprocess.run([H.CLI, "dist", "-q", q, "-r", r, "-o", "out.tsv"] + list(extra), cwd=tmp_path, capture_output=True, text=True,
                          timeout=60)


@pytest.mark.parametrize("other", [["--dm"], ["--top", "3"], ["--max-dist", "0.1"], ["--cluster", "0.05"], ["--derep", "0.05"],
                                   ["--containment", "query"]])
def test_tree_with_another_output_form_is_refused(tmp_path, other):
    for args in (["--tree"] + other, other + ["--tree"], ["--tree", "--linkage", "single"] + other):
        r = _dist(tmp_path, *args)
        assert r.returncode == 2 and "--tree cannot be used with " + other[0] in r.stderr
        assert not (tmp_path / "out.tsv").exists()


def test_linkage_alone_is_refused(tmp_path):
    for other in ([], ["--max-dist", "0.1"], ["--derep", "0.05"], ["--top", "3"], ["--dm"]):
        r = _dist(tmp_path, "--linkage", "average", *other)
        assert r.returncode == 2 and "--linkage needs --tree or --cluster" in r.stderr
        assert not (tmp_path / "out.tsv").exists()


@pytest.mark.parametrize("value", ["", "upgma", "Average", "ward", "0"])
def test_a_bad_linkage_is_refused(tmp_path, value):
    for mode in (["--tree"], ["--cluster", "0.05"], []):
        r = _dist(tmp_path, "--linkage", value, *mode)
        assert r.returncode == 2 and "invalid value '%s' for --linkage" % value in r.stderr
        assert not (tmp_path / "out.tsv").exists()


def test_tree_needs_the_same_files_on_both_sides(tmp_path):
    for q, r_ in (("none", "other"), ("a/none", "a/other")):
        r = _dist(tmp_path, "--tree", q=q, r=r_)
        assert r.returncode == 2 and "--tree needs an all-vs-all run" in r.stderr
        assert not (tmp_path / "out.tsv").exists()


@pytest.mark.parametrize("args", [["--tree"], ["--tree", "--linkage", "average"], ["--tree", "--linkage", "single"],
                                  ["--tree", "--linkage", "complete"], ["--cluster", "0.05", "--linkage", "single"],
                                  ["--cluster", "0.05", "--linkage", "average"], ["--linkage", "complete", "--cluster", "0.05"],
                                  ["--tree", "--fp32", "-m", "0", "--file-order", "--block-rows", "3", "-t", "2", "--devices", "0,0"]])
def test_valid_combinations_are_accepted(tmp_path, args):
    # accepted: the run goes on and fails at the missing sketch files, as it would without the options
    r = _dist(tmp_path, *args)
    want = _dist(tmp_path)
    assert r.returncode == want.returncode == 1 and r.stderr == want.stderr
    assert not (tmp_path / "out.tsv").exists()
    r = _dist(tmp_path, *args, q="./none", r="sub/none")                 # the same files by another spelling
    assert r.returncode == 1 and r.stderr == want.stderr


def test_help_names_tree_and_linkage():
    if not os.path.exists(H.CLI):
        pytest.skip("the lash command line has not been built")
    r = subprocess.run([H.CLI, "--help"], capture_output=True, text=True, timeout=60)
    text = r.stdout + r.stderr
    assert "--tree" in text and "--linkage <average|single|complete>" in text and "Newick" in text
