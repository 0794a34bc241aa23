"""`lash sketch --translate`: what the flag refuses, it refuses before any device is touched — --aa (the input is nucleotide), --min-count,
--window, each with exit 2 and both flag names; a k above 12 (the default 16 included) with the --aa message and exit 101.  The usage text
lists the flag.  No GPU is needed here (FASTQ input is refused when the file is read: tests/test_gpu_translate.py)."""
import os
import subprocess

import pytest

import host_lib as H


def _cli(*args, cwd=None):
    assert os.path.exists(H.CLI), "the lash command line has not been built (build() makes it)"
    return subprocess.run([H.CLI] + list(args), cwd=cwd, capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("extra", [[], ["-k", "7"], ["--per-record"]])
def test_translate_with_aa_is_refused(tmp_path, extra):
    r = _cli("sketch", "-f", "none.txt", "-o", "o", "--translate", "--aa", *extra, cwd=tmp_path)
    assert r.returncode == 2, r.stderr
    assert "--translate" in r.stderr and "--aa" in r.stderr
    assert os.listdir(tmp_path) == []


@pytest.mark.parametrize("extra", [[], ["-k", "7"], ["--count-cells-log2", "20"]])
def test_translate_with_min_count_is_refused(tmp_path, extra):
    r = _cli("sketch", "-f", "none.txt", "-o", "o", "--translate", "--min-count", "2", *extra, cwd=tmp_path)
    assert r.returncode == 2, r.stderr
    assert "--translate" in r.stderr and "--min-count" in r.stderr
    assert os.listdir(tmp_path) == []


@pytest.mark.parametrize("extra", [[], ["-k", "7"], ["--per-record", "-k", "7"]])
def test_translate_with_window_is_refused(tmp_path, extra):
    r = _cli("sketch", "-f", "none.txt", "-o", "o", "--translate", "--window", "1000", *extra, cwd=tmp_path)
    assert r.returncode == 2, r.stderr
    assert "--translate" in r.stderr and "--window" in r.stderr
    assert os.listdir(tmp_path) == []


@pytest.mark.parametrize("extra", [[], ["-k", "13"], ["-k", "32", "--per-record"]])
def test_translate_needs_k_up_to_12(tmp_path, extra):
    r = _cli("sketch", "-f", "none.txt", "-o", "o", "--translate", *extra, cwd=tmp_path)
    want = _cli("sketch", "-f", "none.txt", "-o", "o", "--aa", "-k", "13", cwd=tmp_path)
    assert r.returncode == want.returncode == 101, r.stderr
    assert r.stderr == want.stderr and "amino acid" in r.stderr
    assert os.listdir(tmp_path) == []


@pytest.mark.parametrize("extra", [[], ["--per-record"], ["-a", "ull", "-p", "12"]])
def test_translate_alone_and_with_per_record_is_accepted(tmp_path, extra):
    # accepted: the run goes on and fails at the missing list file, exactly as it would without the flag
    r = _cli("sketch", "-f", "none.txt", "--translate", "-k", "7", *extra, cwd=tmp_path)
    want = _cli("sketch", "-f", "none.txt", "-k", "7", *extra, cwd=tmp_path)
    assert r.returncode == want.returncode == 1 and r.stderr == want.stderr
    assert os.listdir(tmp_path) == []


def test_help_names_translate():
    r = _cli("--help")
    text = r.stdout + r.stderr
    assert "--translate" in text and "-k 1..12" in text
