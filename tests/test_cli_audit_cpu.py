"""CPU: the `niqki` option parser knows --audit and --audit-k (long only, with an argument), and the runs the program
refuses are refused before any work and before any file exists: a bad --audit-k, --audit without a label file of the
run, an index over several GPUs, an engine without niqki_audit (the program is built on the fake engine of
tests/host_san, which answers the C ABI on the CPU without it, as test_cli_lca_cpu.py does, into a path of its own).
Also here, because it needs no device: the product library exports the call, capi.ABI names it and Engine has its
methods."""
import os
import subprocess

import pytest

from conftest import ROOT

HOST = os.path.join(ROOT, "niqki_amd", "host")
OUT = os.path.join(ROOT, "tests", "host_san", "bin", "niqki_fake_audit")
ENGINE = "../../tests/host_san/fake_engine.cpp ../../oracle/niqki_oracle.c"


@pytest.fixture(scope="module")
def niqki_fake():
    subprocess.check_call(["make", "-C", HOST, "-B", "ENGINE=" + ENGINE, "SAN=none", "OUT=" + os.path.relpath(OUT, HOST)],
                          stdout=subprocess.DEVNULL)
    return OUT


def run(binary, args, tmp_path):
    return subprocess.run([binary] + args, cwd=tmp_path, capture_output=True, text=True, timeout=120)


def nothing_written(tmp_path):
    return not (tmp_path / "o.gz").exists() and not (tmp_path / "a.gz").exists()


def test_help_lists_both_options(niqki_fake, tmp_path):
    r = run(niqki_fake, ["--help"], tmp_path)
    assert r.returncode == 0
    text = (r.stderr + r.stdout).splitlines()
    lines = [ln for ln in text if ln.startswith("  --audit ")]
    assert len(lines) == 1 and "<filename>" in lines[0] and "--pan" in lines[0] and "--collapse" in lines[0]
    assert "name<TAB>label<TAB>verdict<TAB>ownName:jaccard<TAB>otherName:jaccard<TAB>otherLabel<TAB>voteLabel:votes" in lines[0]
    assert all(v in lines[0] for v in ("alone", "agrees", "tied", "misplaced", "stray"))
    lines = [ln for ln in text if ln.startswith("  --audit-k ")]
    assert len(lines) == 1 and "<n>" in lines[0] and "1..63" in lines[0] and "(1)" in lines[0]


def test_they_need_their_arguments(niqki_fake, tmp_path):
    (tmp_path / "fof.txt").write_text("")
    for args in (["--audit"], ["--audit="], ["--audit", "a.gz", "--audit-k"], ["--audit", "a.gz", "--audit-k="]):
        r = run(niqki_fake, ["-I", "fof.txt", "-O", "o.gz", "--collapse", "l.txt"] + args, tmp_path)
        assert r.returncode == 1 and "audit" in r.stderr + r.stdout and nothing_written(tmp_path), args


@pytest.mark.parametrize("value", ["0", "64", "-1", "ten", "10x", "1e1", "0.5", " 5", "+5", "99999999999999999999"])
def test_a_bad_audit_k_ends_the_run_before_any_work(niqki_fake, tmp_path, value):
    (tmp_path / "fof.txt").write_text("")
    r = run(niqki_fake, ["-I", "fof.txt", "-O", "o.gz", "--collapse", "l.txt", "--audit", "a.gz", "--audit-k=" + value], tmp_path)
    assert r.returncode == 1 and "audit-k" in r.stderr and "1..63" in r.stderr
    assert "no label audit" not in r.stderr and nothing_written(tmp_path)


def test_a_good_audit_k_is_taken(niqki_fake, tmp_path):
    (tmp_path / "fof.txt").write_text("")
    for value in ("1", "5", "63", "007"):
        r = run(niqki_fake, ["-I", "fof.txt", "-O", "o.gz", "--collapse", "l.txt", "--audit", "a.gz", "--audit-k", value], tmp_path)
        assert r.returncode == 1 and "audit-k" not in r.stderr and "no label audit" in r.stderr   # (the next refusal in line)


def test_audit_needs_the_label_file_of_the_run(niqki_fake, tmp_path):
    (tmp_path / "fof.txt").write_text("")
    for more in ([], ["--audit-k", "3"], ["--lca", "t.txt"], ["--top", "2"]):
        r = run(niqki_fake, ["-I", "fof.txt", "-O", "o.gz", "--audit", "a.gz"] + more, tmp_path)
        assert r.returncode == 1 and "niqki: --audit needs --collapse or --pan" in r.stderr
        assert "no label audit" not in r.stderr and nothing_written(tmp_path)
    # --audit-k alone asks for nothing
    r = run(niqki_fake, ["-I", "fof.txt", "-O", "o.gz", "--audit-k", "3"], tmp_path)
    assert r.returncode == 0 and (tmp_path / "o.gz").exists()


def test_more_than_one_gpu_is_refused_first(niqki_fake, tmp_path):
    for more in (["--collapse", "l.txt"], ["--pan", "l.txt"], []):
        r = run(niqki_fake, ["-I", "fof.txt", "-O", "o.gz", "--gpus", "2", "--audit", "a.gz"] + more, tmp_path)
        assert r.returncode == 1 and "the self-join" in r.stderr and "single-GPU index" in r.stderr
        assert "no label audit" not in r.stderr and "--audit needs" not in r.stderr and nothing_written(tmp_path)


def test_an_engine_without_the_call_says_so(niqki_fake, tmp_path):
    (tmp_path / "fof.txt").write_text("")
    (tmp_path / "l.txt").write_text("")
    for more in ([], ["--audit-k", "2"], ["--lca", "t.txt"]):
        r = run(niqki_fake, ["-I", "fof.txt", "-O", "o.gz", "--collapse", "l.txt", "--audit", "a.gz"] + more, tmp_path)
        assert r.returncode == 1 and "niqki: this engine has no label audit" in r.stderr
        assert nothing_written(tmp_path)                         # before any work
    # beside --pan the engine's first gap is the union itself
    r = run(niqki_fake, ["-I", "fof.txt", "-O", "o.gz", "--pan", "l.txt", "--audit", "a.gz"], tmp_path)
    assert r.returncode == 1 and "niqki: this engine cannot unite genomes" in r.stderr and nothing_written(tmp_path)


def test_the_library_and_the_engine_class_have_the_call(native):
    L = native.lib()
    assert getattr(L, "niqki_audit") is not None
    assert "niqki_audit" in [a[0] for a in native.capi.ABI]
    assert all(callable(getattr(native.Engine, m, None)) for m in ("audit", "audit_dev"))
    assert native.capi.AUDIT_VERDICTS == ("alone", "agrees", "tied", "misplaced", "stray")
    header = open(os.path.join(ROOT, "include", "niqki_hip.h")).read()
    for value, name in enumerate(("ALONE", "AGREES", "TIED", "MISPLACED", "STRAY")):
        assert "#define NIQKI_AUDIT_%s %d\n" % (name, value) in header
        assert getattr(native.capi, "AUDIT_" + name) == value
    assert "#define NIQKI_ABI_VERSION 2 " in header
