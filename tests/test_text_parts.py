"""The text parts of a rank (g-phocs_amd/csrc/gph_textparts.h) and the four joiners over them (gph_textjoin.h: clades, ess,
predictive, triplets), on hand-written parts: no engine, no chain.  2 ranks, 2 samples, loci 0 and 1 on rank 0 and locus 2 on
rank 1.  The good parts join to tests/golden/textparts/ -- what the library wrote for these very parts before the joiners
shared their code -- and every damage below is refused the same way: GPH_EARG, the damaged rank's part named on stderr, no
output file, no part left.

One finding, kept as it was: a part whose last line, the E line, lacks its newline is NOT refused -- the count behind "E\\t"
is read without looking for the end of the line -- and joins to the same files as the good parts (E_WITHOUT_NEWLINE)."""
import os
import subprocess

import pytest

from conftest import GOLDEN, REPO
from sampler_util import hostemu_library

EARG = -1
FORMATS = {   # name: (part suffix, the two outputs)
    "clades": (".clades.part", (".clades.tsv", ".consensus.tsv")),
    "ess": (".ess.part", (".ess.tsv", ".locus-ess.tsv")),
    "predictive": (".predictive.part", (".predictive.tsv", ".predictive-genome.tsv")),
    "triplets": (".triplets.part", (".triplets.tsv", ".triplets-genome.tsv")),
}


def _part(*lines):
    """a part of these lines, the E line counting all but the magic line and an H line"""
    body = [ln for ln in lines[1:] if not ln.startswith("H\t")]
    return "".join(ln + "\n" for ln in lines) + "E\t%d\n" % len(body)


# the good parts: [rank 0, rank 1]
PARTS = {
    "clades": [
        _part("GPHCL1",
              "C\t0\tloc0\t2\t0\t2\t1\t0.5\tA.0,B.1", "T\t0\tloc0\t2\t1\t0\t1\t((A.0,B.1),C.2);",
              "C\t1\tloc1\t2\t0\t2\t0.5\t0.25\tB.1,C.2", "T\t1\tloc1\t2\t2\t0\t0\t(A.0,B.1,C.2);"),
        _part("GPHCL1", "C\t2\tloc2\t2\t1\t2\t1\t0.125\tA.0,C.2", "T\t2\tloc2\t2\t1\t1\t1\t((A.0,C.2),B.1);")],
    "ess": [      # M = 5 series; the P lines are rank 0's alone
        _part("GPHES1", "H\t2\t0\t5",
              "P\ttheta_A\t2\t0.5\t0.25\t2\t2\t1\t0", "P\tFull-ld-ln\t2\t-100.5\t0\t0\t0\t0\t0",
              "P\t# samples 2 level 0 batch 1 minEssAcf 2 (theta_A)",
              "L\t0x1.8p+0\t0\tloc0\t2\t2\t1.5\t2\t2\t2\t1\t1.5", "L\t0x1p+1\t1\tloc1\t2\t2\t2\t2\t2\t2\t0\t2"),
        _part("GPHES1", "H\t2\t0\t5", "L\t0x1p+0\t2\tloc2\t2\t1\t2\t2\t2\t2\t2\t1")],
    "predictive": [      # C = 2 statistics, seed 7
        _part("GPHPD1", "H\t2\t2\t7\tseg\tdiff_A|A",
              "L\t0x1p-1\t0\tloc0\t2\t100\t5\t4.5\t0.7071067812\t0.25\t3\t2.5\t0.7071067812\t0.5\t0.5\tseg",
              "L\t0x1p-2\t1\tloc1\t2\t90\t4\t4\t0\t0.125\t2\t2\t0\t0.5\t0.25\tseg",
              "O\t9\t5", "R\t10\t8\t4", "R\t20\t10\t5"),
        _part("GPHPD1", "H\t2\t2\t7\tseg\tdiff_A|A",
              "L\t0x1p+0\t2\tloc2\t2\t80\t1\t1\t0\t0.5\t1\t1\t0\t0.5\t1\tseg", "O\t1\t1", "R\t10\t1\t2", "R\t20\t1\t0")],
    "triplets": [      # T = 1 triple
        _part("GPHTR1", "H\t2\t1\tA,B,C",
              "L\t0\tloc0\t2\tA\tB\tC\t0.5\t0.25\t0.25\t0.1\t0.2\t0.3\tA,B|C", "L\t1\tloc1\t2\tA\tB\tC\t0.25\t0.5\t0.25\t0.3\t0.2\t0.1\tA,C|B",
              "R\t10\t3\t1\t0", "R\t20\t2\t1\t1"),
        _part("GPHTR1", "H\t2\t1\tA,B,C", "L\t2\tloc2\t2\tA\tB\tC\t1\t0\t0\t0.5\t0\t0\tA,B|C", "R\t10\t1\t0\t0", "R\t20\t0\t0\t1")],
}
STDOUT = {
    "clades": "",
    "ess": "ESS: samples 2 level 0 batch 1 minEssAcf 2 (theta_A); loci 3 level 0 batch 1 medianMinEss 1.5 minMinEss 1 (locus 2)\n",
    "predictive": "Predictive: p\t0.5\t0.25\n",
    "triplets": "Triplets: A,B,C major A,B|C minorA A,C|B minorB B,C|A wMajor 0.6 D 0.3333333333 sd 0.9428090416 pPos 0.5\n",
}


def _lines(text):
    return text.splitlines(keepends=True)


def _edit(parts, rank, fn):
    """rank's part with its lines run through fn(lines) -> lines"""
    out = list(parts)
    out[rank] = "".join(fn(_lines(parts[rank])))
    return out, rank


def _first(lines, tag):
    return next(i for i, ln in enumerate(lines) if ln.startswith(tag))


def _sub(tag, fn):
    """lines -> lines, the first line of that tag rewritten by fn(fields) -> fields"""
    def go(lines):
        i = _first(lines, tag)
        return lines[:i] + ["\t".join(fn(lines[i][:-1].split("\t"))) + "\n"] + lines[i + 1:]
    return go


def _count(by):
    return _sub("E\t", lambda f: [f[0], str(int(f[1]) + by)])


def _has(name, tag):
    return any(ln.startswith(tag) for ln in _lines(PARTS[name][1]))


# damage: name -> fn(format name, good parts) -> (parts, damaged rank), or False where the format has no such line.  A part
# that is None is not written
DAMAGE = {
    "rank 1 absent": lambda n, p: ([p[0], None], 1),
    "empty part": lambda n, p: ([p[0], ""], 1),
    "empty part of rank 0": lambda n, p: (["", p[1]], 0),
    "wrong magic": lambda n, p: _edit(p, 1, lambda ls: ["GPHXX1\n"] + ls[1:]),
    "count one too high": lambda n, p: _edit(p, 1, _count(+1)),
    "count one too low": lambda n, p: _edit(p, 0, _count(-1)),
    "line behind E": lambda n, p: _edit(p, 1, lambda ls: ls + [ls[-2]]),
    "unknown tag": lambda n, p: _edit(p, 1, lambda ls: ls[:-2] + ["Z" + ls[-2][1:]] + ls[-1:]),
    "no E line": lambda n, p: _edit(p, 1, lambda ls: ls[:-1]),
    "cut inside its last line": lambda n, p: _edit(p, 1, lambda ls: ls[:-2] + [ls[-2][:-3]]),
    "H differs in samples": lambda n, p: _has(n, "H\t") and _edit(p, 1, _sub("H\t", lambda f: [f[0], "3"] + f[2:])),
    "H differs in its second field": lambda n, p: _has(n, "H\t") and _edit(p, 1, _sub("H\t", lambda f: f[:2] + [str(int(f[2]) + 1)] + f[3:])),
    "P line on rank 1": lambda n, p: n == "ess" and _edit(p, 1, lambda ls: ls[:2] + ["P\ttheta_A\t2\t0.5\t0.25\t2\t2\t1\t0\n"] + ls[2:-1] + ["E\t2\n"]),
    "L number does not parse": lambda n, p: n in ("ess", "predictive") and _edit(p, 1, _sub("L\t", lambda f: [f[0], "x"] + f[2:])),
    "R iteration differs": lambda n, p: _has(n, "R\t") and _edit(p, 1, _sub("R\t", lambda f: [f[0], "11"] + f[2:])),
    "one R line too few": lambda n, p: _has(n, "R\t") and _edit(p, 1, lambda ls: _count(-1)(ls[:_first(ls, "R\t")] + ls[_first(ls, "R\t") + 1:])),
    "R line one number short": lambda n, p: _has(n, "R\t") and _edit(p, 1, _sub("R\t", lambda f: f[:-1])),
    "non-number in an R line": lambda n, p: _has(n, "R\t") and _edit(p, 1, _sub("R\t", lambda f: f[:-1] + ["x"])),
    "non-number in an O line": lambda n, p: _has(n, "O\t") and _edit(p, 1, _sub("O\t", lambda f: f[:-1] + ["x"])),
}
CASES = [(n, d) for n in FORMATS for d in DAMAGE if DAMAGE[d](n, PARTS[n])]
# not a refusal (see the module's docstring): the E line of rank 1's part without its newline
E_WITHOUT_NEWLINE = lambda n, p: _edit(p, 1, lambda ls: ls[:-1] + [ls[-1][:-1]])      # noqa: E731


@pytest.fixture(scope="module")
def lib():
    return hostemu_library()[1]


def write_parts(name, parts, d):
    """the parts of format `name` under prefix d/out; -> the prefix"""
    os.makedirs(d, exist_ok=True)
    for r, text in enumerate(parts):
        if text is not None:
            open(os.path.join(d, "out" + FORMATS[name][0] + str(r)), "w").write(text)
    return os.path.join(str(d), "out")


def _left(name, prefix):
    """(outputs present, parts present)"""
    sfx, outs = FORMATS[name]
    return [o for o in outs if os.path.exists(prefix + o)], [r for r in range(2) if os.path.exists(prefix + sfx + str(r))]


def _joins_to_the_golden_files(lib, name, parts, d, capfd):
    prefix = write_parts(name, parts, d)
    capfd.readouterr()
    assert getattr(lib, f"gph_{name}_write")(prefix.encode(), 2) == 0
    cap = capfd.readouterr()
    assert cap.out == STDOUT[name] and cap.err == ""
    for o in FORMATS[name][1]:
        assert open(prefix + o).read() == open(os.path.join(GOLDEN, "textparts", "out" + o)).read(), o
    assert _left(name, prefix)[1] == []


@pytest.mark.parametrize("name", list(FORMATS))
def test_good_parts_join(lib, name, tmp_path, capfd):
    _joins_to_the_golden_files(lib, name, PARTS[name], tmp_path, capfd)


@pytest.mark.parametrize("name", list(FORMATS))
def test_an_e_line_without_its_newline_still_joins(lib, name, tmp_path, capfd):
    _joins_to_the_golden_files(lib, name, E_WITHOUT_NEWLINE(name, PARTS[name])[0], tmp_path, capfd)


@pytest.mark.parametrize("name,damage", CASES, ids=[f"{n}-{d.replace(' ', '_')}" for n, d in CASES])
def test_damage_is_refused(lib, name, damage, tmp_path, capfd):
    parts, rank = DAMAGE[damage](name, PARTS[name])
    prefix = write_parts(name, parts, tmp_path)
    capfd.readouterr()
    assert getattr(lib, f"gph_{name}_write")(prefix.encode(), 2) == EARG
    cap = capfd.readouterr()
    assert cap.err == f"gphocs_hip: {prefix}{FORMATS[name][0]}{rank} is missing, damaged or incomplete\n" and cap.out == ""
    assert _left(name, prefix) == ([], [])


@pytest.mark.parametrize("name", list(FORMATS))
def test_discard_removes_parts_and_files(lib, name, tmp_path):
    prefix = write_parts(name, PARTS[name], tmp_path)
    for o in FORMATS[name][1]:
        open(prefix + o, "w").write("x\n")
    assert getattr(lib, f"gph_{name}_discard")(prefix.encode(), 2) == 0
    assert _left(name, prefix) == ([], [])
    assert getattr(lib, f"gph_{name}_discard")(None, 2) == EARG and getattr(lib, f"gph_{name}_write")(None, 2) == EARG
    assert getattr(lib, f"gph_{name}_write")(prefix.encode(), 0) == EARG


def _build_sanitizer_program():
    """tests/hostemu/text_parts_san: its own main() over gph_textjoin.h under AddressSanitizer and
    UndefinedBehaviorSanitizer; rebuilt when a source changes (by content)"""
    import hashlib
    csrc = os.path.join(REPO, "g-phocs_amd", "csrc")
    main = os.path.join(REPO, "tests", "hostemu", "text_parts_san.cpp")
    h = hashlib.sha256()
    for d in [main, os.path.join(csrc, "gph_textjoin.h"), os.path.join(csrc, "gph_textparts.h"), os.path.join(REPO, "include", "gphocs_hip.h")]:
        h.update(os.path.basename(d).encode() + b"\0" + open(d, "rb").read())
    want, exe = h.hexdigest()[:16], os.path.join(REPO, "tests", "hostemu", "text_parts_san")
    try:
        if os.path.exists(exe) and open(exe + ".buildid").read().strip() == want:
            return exe
    except OSError:
        pass
    tmp = f"{exe}.tmp.{os.getpid()}"
    cmd = ["g++", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-O1", "-g", "-std=c++17",
           main, "-o", tmp]
    try:
        subprocess.run(cmd, check=True)
        os.replace(tmp, exe)
    finally:
        if os.path.exists(tmp):
            os.unlink(tmp)
    with open(exe + ".buildid", "w") as f:
        f.write(want + "\n")
    return exe


def test_sanitizer_program(tmp_path):
    """the stand-alone program of tests/hostemu/text_parts_san.cpp over the good parts and every damage above, under
    AddressSanitizer / UndefinedBehaviorSanitizer: a process of its own, nothing of it is loaded into python"""
    exe = _build_sanitizer_program()
    sets = {"good": {n: PARTS[n] for n in FORMATS}, "e_without_newline": {n: E_WITHOUT_NEWLINE(n, PARTS[n])[0] for n in FORMATS}}
    for n, d in CASES:
        sets.setdefault(d.replace(" ", "_"), {})[n] = DAMAGE[d](n, PARTS[n])[0]
    for case, by_format in sets.items():
        for n, parts in by_format.items():
            write_parts(n, parts, tmp_path / case)
    env = {k: v for k, v in os.environ.items() if k != "LD_PRELOAD"}
    r = subprocess.run([exe, str(tmp_path)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    want = f"text_parts_san OK: {len(sets)} directories, 8 joined, {len(CASES)} refused"
    assert want in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stdout + r.stderr
