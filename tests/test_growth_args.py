"""`lash growth`: the arguments are checked before any file is read or any device is touched, so no GPU is needed here."""
import os
import subprocess

import pytest

import host_lib as H


def _growth(tmp_path, *args):
    if not os.path.exists(H.CLI):
        pytest.skip("the lash command line has not been built")
    return subprocess.run([H.CLI, "growth"] + list(args) + ["-o", "out.tsv"], cwd=tmp_path, capture_output=True, text=True, timeout=60)


def _refused(tmp_path, r, text):
    assert r.returncode == 2 and text in r.stderr, r.stderr
    assert not (tmp_path / "out.tsv").exists() and not (tmp_path / "growth").exists()


def test_a_missing_reference_is_refused(tmp_path):
    _refused(tmp_path, _growth(tmp_path), "--reference <reference>")
    _refused(tmp_path, _growth(tmp_path, "--orders", "3"), "--reference <reference>")


@pytest.mark.parametrize("value", ["0", "", "three", "-1", "2.5", "4294967296"])
def test_a_bad_number_of_orders_is_refused(tmp_path, value):
    _refused(tmp_path, _growth(tmp_path, "-r", "none", "--orders", value), "invalid value '%s' for --orders" % value)


def test_both_sources_of_bias_tables_are_refused(tmp_path):
    for args in (["--hll-bias", "t.txt", "--hll-bias-sim"], ["--hll-bias-sim", "--hll-bias=t.txt"]):
        _refused(tmp_path, _growth(tmp_path, "-r", "none", *args), "--hll-bias-sim cannot be used with --hll-bias")


@pytest.mark.parametrize("value", ["", "FGRA", "mle", "0"])
def test_a_bad_estimator_is_refused(tmp_path, value):
    _refused(tmp_path, _growth(tmp_path, "-r", "none", "-e", value), "invalid value '%s' for --estimator" % value)


@pytest.mark.parametrize("other", [["-q", "none"], ["--query", "none"], ["--dm"], ["--top", "3"], ["--max-dist", "0.1"], ["--cluster", "0.05"],
                                   ["--derep", "0.05"], ["--tree"], ["--nj"], ["--linkage", "single"], ["--containment", "query"], ["--fp32"],
                                   ["-m", "0"], ["--block-rows", "3"], ["--devices", "0,0"], ["stray"]])
def test_a_dist_only_flag_is_an_unexpected_argument(tmp_path, other):
    for args in (["-r", "none"] + other, other + ["-r", "none"]):
        _refused(tmp_path, _growth(tmp_path, *args), "unexpected argument '%s'" % other[0])


@pytest.mark.parametrize("args", [[], ["--orders", "1"], ["--orders", "64", "--seed", "7"], ["--file-order", "-e", "ml", "-t", "2", "--device", "0"],
                                  ["--hll-bias-sim"], ["--hll-bias", "t.txt"]])
def test_valid_combinations_are_accepted(tmp_path, args):
    # accepted: the run goes on and fails at the missing sketch files
    r = _growth(tmp_path, "-r", "none", *args)
    assert r.returncode == 1 and "There should be 3 files starting with none" in r.stderr
    assert not (tmp_path / "out.tsv").exists()


def test_help_names_growth():
    if not os.path.exists(H.CLI):
        pytest.skip("the lash command line has not been built")
    r = subprocess.run([H.CLI, "--help"], capture_output=True, text=True, timeout=60)
    text = r.stdout + r.stderr
    assert "growth options:" in text and "--orders <P>" in text and "--seed <S>" in text and "Order<TAB>Step<TAB>Name<TAB>Union<TAB>New" in text
