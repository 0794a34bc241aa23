"""`lash screen`: the arguments are checked before any file is read or any device is touched, so no GPU is needed here."""
import os
import subprocess

import pytest

import host_lib as H


def _screen(tmp_path, *args, output=True):
    assert os.path.exists(H.CLI), "the lash command line has not been built"
    return subprocess.run([H.CLI, "screen"] + list(args) + (["-o", "out.tsv"] if output else []), cwd=tmp_path, capture_output=True, text=True,
                          timeout=60)


def _refused(tmp_path, r, text):
    assert r.returncode == 2 and text in r.stderr, r.stderr
    assert not (tmp_path / "out.tsv").exists()


def test_missing_required_arguments_are_refused(tmp_path):
    _refused(tmp_path, _screen(tmp_path), "--reference <prefix>")
    _refused(tmp_path, _screen(tmp_path, "-q", "none"), "--reference <prefix>")
    _refused(tmp_path, _screen(tmp_path, "-r", "none", "--keep-losers"), "--query <prefix>")
    _refused(tmp_path, _screen(tmp_path, "-r", "none", "-q", "none", output=False), "--output <file>")
    r = _screen(tmp_path, "-r", "none")
    assert "--query <prefix>" in r.stderr and "--reference <prefix>" not in r.stderr and "--output <file>" not in r.stderr


@pytest.mark.parametrize("value", ["nan", "-0.5", "-1e-9", "1.0001", "2", "inf", "-inf", "", "half", "0.5x"])
def test_a_bad_max_dist_is_refused(tmp_path, value):
    _refused(tmp_path, _screen(tmp_path, "-r", "none", "-q", "none", "--max-dist", value), "invalid value '%s' for --max-dist" % value)
    _refused(tmp_path, _screen(tmp_path, "-r", "none", "-q", "none", "--max-dist=" + value), "invalid value '%s' for --max-dist" % value)


@pytest.mark.parametrize("value", ["2", "-1", "poisson", ""])
def test_a_bad_model_is_refused(tmp_path, value):
    _refused(tmp_path, _screen(tmp_path, "-r", "none", "-q", "none", "-m", value), "invalid value '%s' for --model" % value)


@pytest.mark.parametrize("other", [["--dm"], ["--top", "3"], ["--cluster", "0.05"], ["--derep", "0.05"], ["--tree"], ["--nj"], ["--linkage", "single"],
                                   ["--containment", "query"], ["--fp32"], ["-e", "ml"], ["--devices", "0,0"], ["--orders", "3"], ["--keep-others"],
                                   ["--groups", "g.tsv"], ["--all", "x"], ["--core", "0.9"], ["--curves"], ["--hll-bias-sim"], ["stray"]])
def test_a_flag_of_another_command_is_an_unexpected_argument(tmp_path, other):
    for args in (["-r", "none", "-q", "none"] + other, other + ["-r", "none", "-q", "none"]):
        _refused(tmp_path, _screen(tmp_path, *args), "unexpected argument '%s'" % other[0])


@pytest.mark.parametrize("args", [[], ["--max-dist", "0"], ["--max-dist", "1"], ["--max-dist=0.05", "--keep-losers"], ["--max-dist", "1e-3", "-m", "0"],
                                  ["--keep-losers", "--file-order", "-t", "2", "--device", "0", "--block-rows", "3", "-m", "1"]])
def test_valid_combinations_are_accepted(tmp_path, args):
    # accepted: the run goes on and fails at the missing sketch files, with nothing written
    r = _screen(tmp_path, "-r", "none", "-q", "none", *args)
    assert r.returncode == 1 and "There should be 3 files starting with none" in r.stderr, r.stderr
    assert not (tmp_path / "out.tsv").exists()


def test_help_names_screen():
    assert os.path.exists(H.CLI), "the lash command line has not been built"
    r = subprocess.run([H.CLI, "--help"], capture_output=True, text=True, timeout=60)
    text = r.stdout + r.stderr
    assert "screen options:" in text and "--keep-losers" in text and "--max-dist <D>" in text
    assert "Query<TAB>Reference<TAB>Shared<TAB>Won<TAB>Buckets<TAB>Distance<TAB>WtaDistance" in text
