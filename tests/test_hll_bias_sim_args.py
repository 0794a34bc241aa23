"""Arguments of the simulated HLL++ bias tables (`lash hll-bias`, `lash dist --hll-bias-sim`, `lash_amd.allpairs --hll-bias-sim`):
what is refused before any GPU work, and the help texts.  No GPU needed."""
import os
import subprocess
import sys

import host_lib as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lash(tmp_path, *args):
    return subprocess.run([H.CLI] + list(args), cwd=tmp_path, capture_output=True, text=True, timeout=120)


def test_dist_refuses_simulated_tables_together_with_a_file(tmp_path):
    r = _lash(tmp_path, "dist", "-q", "x", "-r", "x", "--hll-bias-sim", "--hll-bias", "x")
    assert r.returncode == 2 and "--hll-bias-sim cannot be used with --hll-bias" in r.stderr
    r = _lash(tmp_path, "dist", "-q", "x", "-r", "x", "--hll-bias=x", "--hll-bias-sim")
    assert r.returncode == 2 and "--hll-bias-sim cannot be used with --hll-bias" in r.stderr


def test_hll_bias_refuses_bad_arguments(tmp_path):
    r = _lash(tmp_path, "hll-bias")
    assert r.returncode == 2 and "--output" in r.stderr
    r = _lash(tmp_path, "hll-bias", "-p", "14")
    assert r.returncode == 2 and "--output" in r.stderr
    for bad in ("3", "19", "14,19", "14,14", "x", ""):
        r = _lash(tmp_path, "hll-bias", "-o", "t.txt", "-p", bad)
        assert r.returncode == 2 and "--precision" in r.stderr, bad
    for bad in ("5", "0", "-7", "x"):
        r = _lash(tmp_path, "hll-bias", "-o", "t.txt", "--points", bad)
        assert r.returncode == 2 and "--points" in r.stderr, bad
    r = _lash(tmp_path, "hll-bias", "-o", "t.txt", "--trials", "0")
    assert r.returncode == 2 and "--trials" in r.stderr
    assert not (tmp_path / "t.txt").exists()


def test_help_texts_name_the_new_flags(tmp_path):
    for args in (("--help",), ("dist", "--help"), ("hll-bias", "--help")):
        r = _lash(tmp_path, *args)
        text = r.stdout + r.stderr
        assert r.returncode == 0, args
        assert "--hll-bias-sim" in text and "hll-bias options:" in text and "--points" in text and "--trials" in text, args
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "lash_amd.allpairs", "--help"], cwd=tmp_path, capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "--hll-bias-sim" in r.stdout
    r = subprocess.run([sys.executable, "-m", "lash_amd.allpairs", "-f", "l.txt", "--hll-bias-sim", "--hll-bias", "x"], cwd=tmp_path,
                       capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 2 and "--hll-bias-sim cannot be used with --hll-bias" in r.stderr
