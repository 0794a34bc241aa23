"""`lash spectrum`: the arguments are checked before any file is read or any device is touched, so no GPU is needed here."""
import os
import subprocess

import pytest

import host_lib as H

OUTPUTS = ("out_spectrum.tsv", "out_groups.tsv", "out_curves.tsv")


def _spectrum(tmp_path, *args, output=True):
    assert os.path.exists(H.CLI), "the lash command line has not been built"
    return subprocess.run([H.CLI, "spectrum"] + list(args) + (["-o", "out"] if output else []), cwd=tmp_path, capture_output=True, text=True,
                          timeout=60)


def _refused(tmp_path, r, text):
    assert r.returncode == 2 and text in r.stderr, r.stderr
    assert not any((tmp_path / f).exists() for f in OUTPUTS)


def test_missing_required_arguments_are_refused(tmp_path):
    _refused(tmp_path, _spectrum(tmp_path), "--reference <prefix>")
    _refused(tmp_path, _spectrum(tmp_path, "--core", "0.9"), "--reference <prefix>")
    _refused(tmp_path, _spectrum(tmp_path, "-r", "none", output=False), "--output <prefix>")


def test_groups_with_all_is_refused(tmp_path):
    (tmp_path / "g.tsv").write_text("g\tm\n")
    _refused(tmp_path, _spectrum(tmp_path, "-r", "none", "--groups", "g.tsv", "--all", "x"), "--groups cannot be used with --all")
    _refused(tmp_path, _spectrum(tmp_path, "-r", "none", "--all", ""), "invalid value '' for --all")


@pytest.mark.parametrize("flag", ["--core", "--cloud"])
@pytest.mark.parametrize("value", ["0", "", "half", "-0.5", "1.0001", "nan", "inf", "0.5x", "2"])
def test_a_bad_fraction_is_refused(tmp_path, flag, value):
    _refused(tmp_path, _spectrum(tmp_path, "-r", "none", flag, value), "invalid value '%s' for %s" % (value, flag))


@pytest.mark.parametrize("args", [["--cloud", "0.96"], ["--core", "0.1"], ["--core", "0.5", "--cloud", "0.6"], ["--cloud=1", "--core=0.99"]])
def test_cloud_above_core_is_refused(tmp_path, args):
    _refused(tmp_path, _spectrum(tmp_path, "-r", "none", *args), "--cloud must not be above --core")


@pytest.mark.parametrize("other", [["-q", "none"], ["--query", "none"], ["--dm"], ["--top", "3"], ["--max-dist", "0.1"], ["--cluster", "0.05"],
                                   ["--derep", "0.05"], ["--tree"], ["--nj"], ["--linkage", "single"], ["--containment", "query"], ["--fp32"],
                                   ["-m", "0"], ["-e", "ml"], ["--block-rows", "3"], ["--devices", "0,0"], ["--orders", "3"], ["--keep-others"],
                                   ["--hll-bias-sim"], ["stray"]])
def test_a_flag_of_another_command_is_an_unexpected_argument(tmp_path, other):
    for args in (["-r", "none"] + other, other + ["-r", "none"]):
        _refused(tmp_path, _spectrum(tmp_path, *args), "unexpected argument '%s'" % other[0])


@pytest.mark.parametrize("args", [[], ["--all", "pan"], ["--core", "1", "--cloud", "1"], ["--core", "0.9", "--cloud", "0.9"], ["--cloud", "1e-3"],
                                  ["--curves", "--file-order", "-t", "2", "--device", "0"], ["--groups", "missing.tsv"]])
def test_valid_combinations_are_accepted(tmp_path, args):
    # accepted: the run goes on and fails at the missing sketch files, with nothing written
    r = _spectrum(tmp_path, "-r", "none", *args)
    assert r.returncode == 1 and "There should be 3 files starting with none" in r.stderr, r.stderr
    assert not any((tmp_path / f).exists() for f in OUTPUTS)


def test_help_names_spectrum():
    assert os.path.exists(H.CLI), "the lash command line has not been built"
    r = subprocess.run([H.CLI, "--help"], capture_output=True, text=True, timeout=60)
    text = r.stdout + r.stderr
    assert "spectrum options:" in text and "--core <F>" in text and "--cloud <F>" in text and "--curves" in text
    assert "Group<TAB>Members<TAB>Count<TAB>Buckets<TAB>Kmers" in text and "Group<TAB>Members<TAB>Occupied<TAB>Union<TAB>Core<TAB>Shell<TAB>Cloud" in text
