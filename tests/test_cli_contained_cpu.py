"""CPU: the `niqki` option parser knows --min-containment and --containment-of (long only, their values checked before
any work), and a host program built on an engine without niqki_set_sizes / niqki_staged_query_contained says so before
any work: the program is built on the fake engine of tests/host_san (the C ABI answered on the CPU, the calls not among
its symbols), as test_cli_sizes_cpu.py does, into its own path.  The combinations the program refuses on its own are
refused first."""
import os
import subprocess

import pytest

from conftest import ROOT

HOST = os.path.join(ROOT, "niqki_amd", "host")
OUT = os.path.join(ROOT, "tests", "host_san", "bin", "niqki_fake_contained")
ENGINE = "../../tests/host_san/fake_engine.cpp ../../oracle/niqki_oracle.c"
LACKS = "niqki: this engine cannot select hits by containment"


@pytest.fixture(scope="module")
def niqki_fake():
    subprocess.check_call(["make", "-C", HOST, "-B", "ENGINE=" + ENGINE, "SAN=none", "OUT=" + os.path.relpath(OUT, HOST)],
                          stdout=subprocess.DEVNULL)
    return OUT


def run(binary, args, tmp_path):
    return subprocess.run([binary] + args, cwd=tmp_path, capture_output=True, text=True, timeout=120)


def test_help_lists_both_options(niqki_fake, tmp_path):
    r = run(niqki_fake, ["--help"], tmp_path)
    text = r.stderr + r.stdout
    assert r.returncode == 0 and "--min-containment <x>" in text and "--containment-of <which>" in text
    assert "-J stays the floor" in text and "query" in text and "genome" in text and "either" in text


def test_min_containment_needs_a_value(niqki_fake, tmp_path):
    r = run(niqki_fake, ["-Q", "fof.txt", "--min-containment"], tmp_path)
    assert r.returncode == 1 and "Option 'min-containment' requires a non-empty argument" in r.stderr
    r = run(niqki_fake, ["-Q", "fof.txt", "--min-containment="], tmp_path)
    assert r.returncode == 1 and "requires a non-empty argument" in r.stderr


@pytest.mark.parametrize("value", ["0", "1.5", "x", "-0.5", "0.5x", "nan", "1.0000001", " 0.5", ""])
def test_min_containment_takes_a_share_above_0_up_to_1(niqki_fake, tmp_path, value):
    (tmp_path / "fof.txt").write_text("")
    r = run(niqki_fake, ["-I", "fof.txt", "-O", "o.gz", "-D", "d.dump", "-Q", "fof.txt", "--min-containment=" + value], tmp_path)
    assert r.returncode == 1 and ("Option 'min-containment' requires" in r.stderr) and "Bad usage!!!" in r.stdout
    assert not any((tmp_path / f).exists() for f in ("o.gz", "d.dump"))               # before any work


def test_containment_of_needs_min_containment_and_a_known_word(niqki_fake, tmp_path):
    (tmp_path / "fof.txt").write_text("")
    base = ["-I", "fof.txt", "-O", "o.gz", "-Q", "fof.txt"]
    r = run(niqki_fake, base + ["--containment-of", "genome"], tmp_path)
    assert r.returncode == 1 and "--containment-of needs --min-containment" in r.stderr
    r = run(niqki_fake, base + ["--containment-of"], tmp_path)
    assert r.returncode == 1 and "Option 'containment-of' requires a non-empty argument" in r.stderr
    for word in ("both", "Query", "0"):
        r = run(niqki_fake, base + ["--min-containment", "0.5", "--containment-of", word], tmp_path)
        assert r.returncode == 1 and "Option 'containment-of' requires query, genome or either" in r.stderr, word
    assert not (tmp_path / "o.gz").exists()


def test_the_options_are_long_only(niqki_fake, tmp_path):
    for wrong in ("--min-contain", "--mincontainment", "--containment_of"):
        r = run(niqki_fake, [wrong, "0.5"], tmp_path)
        assert r.returncode == 1 and "Unknown option '%s'" % wrong[2:] in r.stderr
    # the help names no short form (as in "  --index, -I <filename>")
    lines = (lambda r: (r.stderr + r.stdout).splitlines())(run(niqki_fake, ["--help"], tmp_path))
    assert any(x.startswith("  --min-containment <x>  ") for x in lines) and any(x.startswith("  --containment-of <which>  ") for x in lines)


@pytest.mark.parametrize("of", ([], ["--containment-of", "query"], ["--containment-of", "genome"], ["--containment-of", "either"]))
def test_an_engine_without_the_calls_says_so(niqki_fake, tmp_path, of):
    (tmp_path / "fof.txt").write_text("")
    for x in ("0.8", "1", "1e-9"):
        r = run(niqki_fake, ["-I", "fof.txt", "-O", "o.gz", "-D", "d.dump", "-Q", "fof.txt", "--min-containment", x] + of, tmp_path)
        assert r.returncode == 1 and LACKS in r.stderr
        assert not any((tmp_path / f).exists() for f in ("o.gz", "d.dump"))           # before any work


@pytest.mark.parametrize("other, text", ((["--cover"], "--cover"), (["--collapse", "g.tsv"], "--collapse"), (["--lca", "t.tsv"], "--lca"),
                                         (["--gpus", "2"], "single-GPU index")))
def test_the_refused_combinations_are_refused_first(niqki_fake, tmp_path, other, text):
    (tmp_path / "fof.txt").write_text("")
    r = run(niqki_fake, ["-I", "fof.txt", "-O", "o.gz", "--min-containment", "0.8", "-Q", "fof.txt"] + other, tmp_path)
    assert r.returncode == 1 and text in r.stderr and "--min-containment" in r.stderr and "by containment" not in r.stderr
    assert not (tmp_path / "o.gz").exists()
