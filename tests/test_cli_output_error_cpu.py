"""CPU: a run whose output cannot be written ends with ONE message and exit code 1, not with an abort.  The writer keeps
text until it is closed, so after an error that main has already reported the destructor of the index closes a writer
with text pending on a file that takes none (/dev/full): that second failure must stay inside the destructor.  The
program is built on the fake engine of tests/host_san, as test_cli_cover_cpu.py does, into a path of its own."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

HOST = os.path.join(ROOT, "niqki_amd", "host")
OUT = os.path.join(ROOT, "tests", "host_san", "bin", "niqki_fake_output_error")
ENGINE = "../../tests/host_san/fake_engine.cpp ../../oracle/niqki_oracle.c"


@pytest.fixture(scope="module")
def niqki_fake():
    subprocess.check_call(["make", "-C", HOST, "-B", "ENGINE=" + ENGINE, "SAN=none", "OUT=" + os.path.relpath(OUT, HOST)],
                          stdout=subprocess.DEVNULL)
    return OUT


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    td = tmp_path_factory.mktemp("output_error")
    rng = np.random.default_rng(7)
    names = []
    for g in range(4):
        seq = "".join("ACGT"[c] for c in rng.integers(0, 4, 3000))
        (td / ("g%d.fa" % g)).write_text(">g%d\n%s\n" % (g, seq))
        names.append("g%d.fa" % g)
    (td / "fof.txt").write_text("\n".join(names) + "\n")
    return td


def run(binary, args, td):
    return subprocess.run([binary] + args, cwd=td, capture_output=True, text=True, timeout=120)


def test_an_error_with_text_pending_exits_1(niqki_fake, workdir):
    """The hits of -Q are pending in the writer when -l fails to open its file: main reports that error, and the
    destructor's close fails on /dev/full.  (The parent of this change ended here with SIGABRT: return code -6.)"""
    r = run(niqki_fake, ["-I", "fof.txt", "-Q", "fof.txt", "-l", "no_such.fa", "-S", "10", "-O", "/dev/full"], workdir)
    assert r.returncode == 1, (r.returncode, r.stderr)
    assert "terminate called" not in r.stderr
    assert "niqki: cannot open 'no_such.fa'" in r.stderr


def test_a_failed_write_exits_1(niqki_fake, workdir):
    r = run(niqki_fake, ["-I", "fof.txt", "-Q", "fof.txt", "-S", "10", "-O", "/dev/full"], workdir)
    assert r.returncode == 1, (r.returncode, r.stderr)
    assert "terminate called" not in r.stderr
    assert "niqki: write failed" in r.stderr
