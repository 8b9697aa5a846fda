"""CPU: the `niqki` option parser knows --top (long only, numeric, not negative).  The host program is built on the
fake engine of tests/host_san (the C ABI answered on the CPU), as test_host_sanitizers.py does, into its own path."""
import os
import subprocess

import pytest

from conftest import ROOT

HOST = os.path.join(ROOT, "niqki_amd", "host")
OUT = os.path.join(ROOT, "tests", "host_san", "bin", "niqki_fake_topk")
ENGINE = "../../tests/host_san/fake_engine.cpp ../../oracle/niqki_oracle.c"


@pytest.fixture(scope="module")
def niqki_fake():
    subprocess.check_call(["make", "-C", HOST, "-B", "ENGINE=" + ENGINE, "SAN=none", "OUT=" + os.path.relpath(OUT, HOST)],
                          stdout=subprocess.DEVNULL)
    return OUT


def run(binary, args, tmp_path):
    return subprocess.run([binary] + args, cwd=tmp_path, capture_output=True, text=True, timeout=120)


def test_help_lists_top(niqki_fake, tmp_path):
    r = run(niqki_fake, ["--help"], tmp_path)
    assert r.returncode == 0
    assert "--top <int>" in r.stderr + r.stdout
    assert "Report at most <int> best hits per query (0: all)." in r.stderr + r.stdout


def test_top_needs_a_number(niqki_fake, tmp_path):
    r = run(niqki_fake, ["-I", "fof.txt", "--top", "x"], tmp_path)
    assert r.returncode == 1 and "Option 'top' requires a numeric argument" in r.stderr
    r = run(niqki_fake, ["-I", "fof.txt", "--top", "-1"], tmp_path)
    assert r.returncode == 1 and "Option 'top'" in r.stderr
    r = run(niqki_fake, ["-I", "fof.txt", "-t", "3"], tmp_path)   # long only: no short form
    assert r.returncode == 1
