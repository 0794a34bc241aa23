"""`lash sketch --window W`: what the flag refuses, it refuses before any device is touched — a W that is no positive integer, a W
shorter than k, --aa, --min-count.  The usage text lists the flag.  No GPU is needed here (FASTQ input is refused when the file is read, which a run
without a device never gets to: tests/test_gpu_windows.py)."""
import os
import subprocess

import pytest

import host_lib as H


def _cli(*args, cwd=None):
    assert os.path.exists(H.CLI), "the lash command line has not been built (build() makes it)"
    return subprocess.run([H.CLI] + list(args), cwd=cwd, capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("w", ["0", "-5", "abc", "1.5", "", "10k"])
def test_window_must_be_a_positive_integer(tmp_path, w):
    r = _cli("sketch", "-f", "none.txt", "-o", "o", "--window", w, cwd=tmp_path)
    assert r.returncode == 2, r.stderr
    assert "--window" in r.stderr and "positive integer" in r.stderr
    assert os.listdir(tmp_path) == []


@pytest.mark.parametrize("extra,w", [([], "15"), (["-k", "21"], "20"), (["-k", "32", "-a", "ull"], "1")])
def test_window_shorter_than_k_is_refused(tmp_path, extra, w):
    r = _cli("sketch", "-f", "none.txt", "-o", "o", "--window", w, *extra, cwd=tmp_path)
    assert r.returncode == 2, r.stderr
    assert "--window" in r.stderr and "-k" in r.stderr
    assert os.listdir(tmp_path) == []


@pytest.mark.parametrize("extra", [[], ["-k", "8"], ["--per-record"]])
def test_window_with_aa_is_refused(tmp_path, extra):
    r = _cli("sketch", "-f", "none.txt", "-o", "o", "--window", "1000", "--aa", "-k", "8", *extra, cwd=tmp_path)
    assert r.returncode == 2, r.stderr
    assert "--window" in r.stderr and "--aa" in r.stderr
    assert os.listdir(tmp_path) == []


@pytest.mark.parametrize("extra", [[], ["--count-cells-log2", "20"]])
def test_window_with_min_count_is_refused(tmp_path, extra):
    r = _cli("sketch", "-f", "none.txt", "-o", "o", "--window", "1000", "--min-count", "2", *extra, cwd=tmp_path)
    assert r.returncode == 2, r.stderr
    assert "--window" in r.stderr and "--min-count" in r.stderr
    assert os.listdir(tmp_path) == []


@pytest.mark.parametrize("extra", [[], ["--per-record"], ["-k", "16"]])
def test_window_alone_and_with_per_record_is_accepted(tmp_path, extra):
    # accepted (W == k included): the run goes on and fails at the missing list file, as it would without the flag
    r = _cli("sketch", "-f", "none.txt", "--window", "16", *extra, cwd=tmp_path)
    want = _cli("sketch", "-f", "none.txt", cwd=tmp_path)
    assert r.returncode == want.returncode == 1 and r.stderr == want.stderr


def test_help_names_window():
    r = _cli("--help")
    assert "--window" in r.stdout + r.stderr

