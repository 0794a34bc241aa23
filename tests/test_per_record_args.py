"""`lash sketch --per-record`: the flag is refused with --aa before any file is read or any device is touched, and the usage text lists
it, so no GPU is needed here."""
import os
import subprocess

import pytest

import host_lib as H


def _cli(*args, cwd=None):
    assert os.path.exists(H.CLI), "the lash command line has not been built (build() makes it)"
    return subprocess.run([H.CLI] + list(args), cwd=cwd, capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("extra", [[], ["-k", "8"], ["-k", "16", "-a", "ull"]])
def test_per_record_with_aa_is_refused(tmp_path, extra):
    r = _cli("sketch", "-f", "none.txt", "-o", "o", "--per-record", "--aa", *extra, cwd=tmp_path)
    assert r.returncode == 2, r.stderr
    assert "--per-record" in r.stderr and "--aa" in r.stderr
    assert os.listdir(tmp_path) == []


def test_per_record_alone_is_accepted(tmp_path):
    # accepted: the run goes on and fails at the missing list file, as it would without the flag
    r = _cli("sketch", "-f", "none.txt", "--per-record", cwd=tmp_path)
    want = _cli("sketch", "-f", "none.txt", cwd=tmp_path)
    assert r.returncode == want.returncode == 1 and r.stderr == want.stderr


def test_help_names_per_record():
    r = _cli("--help")
    assert "--per-record" in r.stdout + r.stderr
