"""CPU: every `Name.java:N[-M]` citation in the product, oracle and host code
resolves against the reference sources (the file exists, every cited line is
inside it), and where a cited line carries a message or output literal, the
literal is on the cited lines.

The reference sources are not part of this repository, so the tests read an
index of them, tests/golden/reference_index.json: the line count of every
reference file, and one hash for every (file, cited lines, literal) that was
found on its cited lines when the index was made. A citation moved to
another line, or a new one, is not in the index and fails until
tests/golden/make_reference_index.py is run against the reference sources
again (it refuses a literal that is not on the lines cited for it)."""
import hashlib
import json
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INDEX = os.path.join(ROOT, "tests", "golden", "reference_index.json")
SCANNED = ["include", "oracle", "genome.distance_amd/gdist", "genome.distance_amd/csrc", "tests",
           "INTEGRATION.md", "DESIGN.md", "bench.py", "__graft_entry__.py"]
CITE = re.compile(r"([A-Za-z]+\.java):(\d+(?:-\d+)?(?:,\s?\d+(?:-\d+)?)*)")
LITERAL = re.compile(r'"((?:[^"\\]|\\.){12,})"')


def _index():
    with open(INDEX) as f:
        return json.load(f)


def _sources():
    for entry in SCANNED:
        p = os.path.join(ROOT, entry)
        if os.path.isfile(p):
            yield p
            continue
        for dirpath, _, files in os.walk(p):
            for fn in files:
                if fn.endswith((".py", ".h", ".hip", ".hpp", ".c", ".md")):
                    yield os.path.join(dirpath, fn)


def _ranges(spec):
    for part in spec.split(","):
        a, _, b = part.strip().partition("-")
        yield int(a), int(b or a)


def _citations():
    for path in _sources():
        with open(path, errors="replace") as f:
            for ln, line in enumerate(f, 1):
                for m in CITE.finditer(line):
                    yield path, ln, line, m.group(1), list(_ranges(m.group(2)))


def _cited_literals():
    """(path, line number, reference file, cited ranges, literal, probe) of
    every host-code line that raises a reference message or writes a
    reference header and cites the reference line it follows; the probe is
    the part of the literal that must stand on the cited lines."""
    for path, ln, line, name, ranges in _citations():
        if not path.endswith(".py") or not ("raise " in line or ".write(" in line):
            continue
        for lit in LITERAL.findall(line):
            if lit.startswith(("{", "%")):
                continue
            probe = lit.split("{")[0].replace("\\n", "")[:40]
            if len(probe) >= 8:
                yield path, ln, name, ranges, lit, probe


def literal_key(name, ranges, probe):
    spec = ",".join(f"{a}-{b}" for a, b in ranges)
    return hashlib.sha256(f"{name}:{spec}:{probe}".encode()).hexdigest()[:20]


def test_citations_resolve():
    lines = _index()["lines"]
    bad, n = [], 0
    for path, ln, _, name, ranges in _citations():
        n += 1
        rel = os.path.relpath(path, ROOT)
        if name not in lines:
            bad.append(f"{rel}:{ln}: {name} is not a reference file")
            continue
        nlines = lines[name]
        for a, b in ranges:
            if not (1 <= a <= b <= nlines):
                bad.append(f"{rel}:{ln}: {name}:{a}-{b} outside its {nlines} lines")
    assert n > 50, "citation scan found too few citations"
    assert not bad, "\n".join(bad)


def test_cited_literals_are_on_the_cited_lines():
    """A host-code line that raises a reference message or writes a reference
    header, and cites the reference line it follows, must cite the line that
    holds that text (catches citations shifted to a wrong but existing line)."""
    idx = _index()
    found = set(idx["literals_on_cited_lines"])
    bad, checked = [], 0
    for path, ln, name, ranges, lit, probe in _cited_literals():
        if name not in idx["lines"]:
            continue
        checked += 1
        if literal_key(name, ranges, probe) not in found:
            bad.append(f"{os.path.relpath(path, ROOT)}:{ln}: {lit!r} not on {name}:{ranges}")
    assert checked >= 8, f"only {checked} cited literals found"
    assert not bad, "\n".join(bad)
