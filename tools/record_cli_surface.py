#!/usr/bin/env python3
"""Records what a `lash` binary answers to every command line of tests/cli_cases.py:

    python tools/record_cli_surface.py BINARY tests/golden/cli_surface.json

Each case runs in a fresh empty directory, without LASH_HLL_BIAS, LASH_LAYOUT and LASH_CLI_TIMING; its exit code, stdout and stderr
go to the JSON file tests/test_cli_surface.py compares the built binary with.  Record it from the commit BEFORE a change to the
command-line layer and commit it unchanged with that change."""
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from cli_cases import CASES  # noqa: E402

SCRUBBED = ("LASH_HLL_BIAS", "LASH_LAYOUT", "LASH_CLI_TIMING")
# an accepted case has to stop at an input that is not there, before any device is opened
MISSING_INPUT = ("There should be 3 files starting with", "cannot open list file")


def run_case(binary, args):
    env = {k: v for k, v in os.environ.items() if k not in SCRUBBED}
    with tempfile.TemporaryDirectory() as cwd:
        r = subprocess.run([binary] + args, cwd=cwd, env=env, capture_output=True, text=True, timeout=60)
        left = os.listdir(cwd)
    return {"args": args, "exit": r.returncode, "stdout": r.stdout, "stderr": r.stderr, "files": left}


def touches_no_gpu(rec):
    """why the record shows that no device was opened, or None"""
    if rec["files"]:
        return None
    if rec["exit"] in (2, 101):
        return "refused"
    if rec["exit"] == 1 and any(m in rec["stderr"] for m in MISSING_INPUT):
        return "missing input"
    if rec["exit"] == 0 and ("Usage: lash <COMMAND>" in rec["stderr"] or rec["args"][:1] in (["-V"], ["--version"])):
        return "help or version"
    return None


def load(path):
    """the records of a file main() wrote: a stdout or stderr that is a number stands for that entry of "shared" """
    with open(path) as f:
        doc = json.load(f)
    text = lambda v: doc["shared"][v] if isinstance(v, int) else v
    return [{"args": a, "exit": rc, "stdout": text(out), "stderr": text(err)} for a, rc, out, err in doc["cases"]]


def main():
    binary, out = os.path.abspath(sys.argv[1]), sys.argv[2]
    records = [run_case(binary, args) for args in CASES]
    bad = [r for r in records if touches_no_gpu(r) is None]
    for r in bad:
        print("not a case for this corpus (it may open a device or it wrote a file): %r -> exit %d\n%s" % (r["args"], r["exit"], r["stderr"]))
    if bad:
        return 1
    # one line per case; a text that several cases print (the banner, the usage, a missing input) is written once
    texts = [r[k] for r in records for k in ("stdout", "stderr")]
    shared = sorted({t for t in texts if texts.count(t) > 1})
    ref = lambda t: shared.index(t) if t in shared else t
    lines = [json.dumps([r["args"], r["exit"], ref(r["stdout"]), ref(r["stderr"])], ensure_ascii=False) for r in records]
    with open(out, "w") as f:
        f.write('{"shared": [\n' + ",\n".join(json.dumps(t, ensure_ascii=False) for t in shared) + '\n],\n"cases": [\n' + ",\n".join(lines) + "\n]}\n")
    assert [dict(r, files=[]) for r in load(out)] == records
    print("%d cases recorded in %s" % (len(records), out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
