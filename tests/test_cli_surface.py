"""The whole command-line surface of `lash`, byte for byte: exit code, stdout and stderr of every command line of cli_cases.py
against tests/golden/cli_surface.json, which tools/record_cli_surface.py wrote from the binary of the commit before the
command-line layer was last reworked.  Every case ends before a device is opened (it is refused, it is --help, or it fails on an
input that is not there), so no GPU is needed here."""
import os
import sys

import pytest

import host_lib as H
from cli_cases import CASES

sys.path.insert(0, os.path.join(H.ROOT, "tools"))
import record_cli_surface as R  # noqa: E402

GOLDEN = R.load(os.path.join(H.ROOT, "tests", "golden", "cli_surface.json"))


def test_the_record_and_the_cases_are_the_same_list():
    assert [g["args"] for g in GOLDEN] == CASES


def test_no_recorded_case_opened_a_device():
    for g in GOLDEN:
        assert R.touches_no_gpu(dict(g, files=[])) is not None, g["args"]
    assert not any(g["args"][:1] == ["hll-bias"] and g["exit"] not in (0, 2) for g in GOLDEN)


@pytest.mark.parametrize("chunk", range(8))
def test_every_case_answers_as_recorded(chunk):
    assert os.path.exists(H.CLI), "the lash command line has not been built"
    differ = []
    for want in GOLDEN[chunk::8]:
        got = R.run_case(H.CLI, want["args"])
        for field in ("exit", "stdout", "stderr"):
            if got[field] != want[field]:
                differ.append("lash %s: %s\n  recorded: %r\n  now:      %r" % (" ".join(want["args"]), field, want[field], got[field]))
        if got["files"]:
            differ.append("lash %s wrote %r" % (" ".join(want["args"]), got["files"]))
    assert not differ, "%d differences\n%s" % (len(differ), "\n".join(differ))
