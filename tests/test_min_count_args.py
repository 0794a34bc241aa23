"""`lash sketch --min-count`: the argument errors leave with exit code 2 and say why, before any GPU is touched."""
import subprocess

import pytest

import host_lib as H


def run(tmp_path, *extra):
    lst = tmp_path / "list.txt"
    lst.write_text("")
    return subprocess.run([H.CLI, "sketch", "-f", str(lst), "-o", str(tmp_path / "o")] + list(extra), capture_output=True, text=True)


@pytest.mark.parametrize("extra,text", [
    (["--min-count", "0"], "--min-count: an integer from 1 to 255"),
    (["--min-count", "256"], "--min-count: an integer from 1 to 255"),
    (["--min-count", "two"], "--min-count: an integer from 1 to 255"),
    (["--min-count", "-1"], "--min-count: an integer from 1 to 255"),
    (["--min-count", "2.5"], "--min-count: an integer from 1 to 255"),
    (["--min-count", "2", "--count-cells-log2", "9"], "--count-cells-log2: an integer from 10 to 36"),
    (["--min-count", "2", "--count-cells-log2", "37"], "--count-cells-log2: an integer from 10 to 36"),
    (["--count-cells-log2", "20"], "--count-cells-log2 needs --min-count"),
    (["--min-count", "2", "--aa", "-k", "8"], "--min-count cannot be used with --aa"),
    (["--min-count", "2", "--per-record"], "--min-count cannot be used with --per-record"),
    (["--min-count", "2", "-a", "hll", "-p", "16"], "--min-count supports -a hll up to -p 15"),
    (["--min-count", "2", "-a", "ull", "-p", "15"], "--min-count supports -a ull up to -p 14"),
])
def test_argument_errors(tmp_path, extra, text):
    r = run(tmp_path, *extra)
    assert r.returncode == 2, (r.returncode, r.stderr)
    assert text in r.stderr


def test_help_mentions_the_flag():
    r = subprocess.run([H.CLI, "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    assert "--min-count <M>" in r.stderr and "--count-cells-log2 <L>" in r.stderr
    r = subprocess.run([H.CLI, "sketch", "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--min-count <M>" in r.stderr
