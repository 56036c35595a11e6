"""tests/option_cases.py cannot fall behind the library (no GPU, no library
load): its keys are exactly the names of GDIST_OPTIONS in
csrc/gdist_internal.hpp, every covered_by target exists and names its option,
and every sweep value is a parameter id of tests/test_gpu_option_sweep.py."""
import ast
import importlib
import os
import re

from option_cases import OPTIONS, SCENE_K, SCENE_S, SCENE_T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HPP = os.path.join(ROOT, "genome.distance_amd", "csrc", "gdist_internal.hpp")
SWEEP_FILE = "tests/test_gpu_option_sweep.py"
KINDS = ("covered_by", "sweep", "exempt")


def library_options(text=None):
    """The names in the GDIST_OPTIONS(X) macro, in order."""
    text = open(HPP).read() if text is None else text
    m = re.search(r"#define GDIST_OPTIONS\(X\)(.*?)\n\s*\n", text, re.S)
    assert m, "GDIST_OPTIONS(X) not found"
    names = re.findall(r'\bX\(\s*([A-Z0-9_]+)\s*,\s*"([a-z0-9_]+)"\s*\)', m.group(1))
    assert len(names) > 50 and m.group(1).count("X(") == len(names), "an X(...) row the pattern does not read"
    for ident, name in names:
        assert ident.lower() == name, (ident, name)
    return [name for _, name in names]


def table_problems(options, names):
    """What keeps `options` from being the table of `names` (empty: nothing)."""
    out = []
    for n in names:
        if n not in options:
            out.append(f"option {n} has no entry in tests/option_cases.py")
    for n in options:
        if n not in names:
            out.append(f"entry {n} names no option of GDIST_OPTIONS")
    for n, e in options.items():
        if sorted(e) not in ([k] for k in KINDS):
            out.append(f"entry {n}: exactly one of {KINDS}, not {sorted(e)}")
    return out


def test_table_keys_are_the_library_options():
    names = library_options()
    assert len(set(names)) == len(names)
    assert table_problems(OPTIONS, names) == []
    for n, e in OPTIONS.items():
        if "exempt" in e:
            assert isinstance(e["exempt"], str) and len(e["exempt"]) > 20 and "\n" not in e["exempt"], n
        else:
            assert list(e.values())[0], (n, "no target or value")


def module_sources(path):
    """Top-level functions and assignments of a test file: name -> source."""
    text = open(os.path.join(ROOT, path)).read()
    out = {}
    for node in ast.parse(text).body:
        seg = ast.get_source_segment(text, node)
        if isinstance(node, (ast.FunctionDef, ast.AsyncFunctionDef)):
            out[node.name] = seg
        elif isinstance(node, ast.Assign):
            for t in node.targets:
                if isinstance(t, ast.Name):
                    out[t.id] = seg
    return out


def reachable_source(sources, func):
    """The function's source with that of the module-level tables and helpers
    it names (SPARSE_MODES, run_variants -> VARIANTS, ...)."""
    seen, todo, text = set(), [func], []
    while todo:
        name = todo.pop()
        if name in seen or name not in sources:
            continue
        seen.add(name)
        text.append(sources[name])
        for ident in set(re.findall(r"[A-Za-z_][A-Za-z0-9_]*", sources[name])):
            if ident in sources and not ident.startswith("test_"):
                todo.append(ident)
    return "\n".join(text)


def test_covered_by_targets_exist_and_name_their_option():
    cache, reach = {}, {}
    for n, e in OPTIONS.items():
        for (path, func, values) in e.get("covered_by", []):
            assert values, (n, path, func, "no value listed")
            assert os.path.exists(os.path.join(ROOT, path)), (n, path)
            assert path != SWEEP_FILE, (n, "the sweep file's options are `sweep` entries")
            if path not in cache:
                cache[path] = module_sources(path)
            src = cache[path]
            assert func in src, (n, path, func)
            if (path, func) not in reach:
                reach[path, func] = reachable_source(src, func)
            assert re.search(r"\b%s\b" % re.escape(n), reach[path, func]), \
                f"{path}::{func} never names option {n}"


def sweep_ids():
    """Parameter ids of the sweep file's tests (the ids its parametrize marks
    carry: read from the marks, no test is run)."""
    mod = importlib.import_module("test_gpu_option_sweep")
    ids = []
    for name in dir(mod):
        fn = getattr(mod, name)
        if not name.startswith("test_") or not callable(fn):
            continue
        for mark in getattr(fn, "pytestmark", []):
            if mark.name != "parametrize":
                continue
            got = mark.kwargs.get("ids")
            values = mark.args[1]
            ids += [got(v) for v in values] if callable(got) else list(got)
    return ids


def test_sweep_values_are_parameter_ids():
    ids = sweep_ids()
    assert len(ids) == len(set(ids)) == len(SCENE_K) + sum(len(w) for _, w in SCENE_S) + sum(map(len, SCENE_T.values()))
    for n, e in OPTIONS.items():
        for v in e.get("sweep", []):
            pat = re.compile(r"(^|,)%s=%d(,|@|$)" % (re.escape(n), v))
            assert any(pat.search(i) for i in ids), f"{SWEEP_FILE} has no case with {n}={v}"
    # and nothing is swept that the table does not say: every option of a
    # case's own dict is a sweep entry or covered elsewhere (a helper setting)
    rows = [o for _, o, _ in SCENE_K] + [o for o, _ in SCENE_S] + [o for t in SCENE_T.values() for o in t]
    for o in rows:
        for k in o:
            assert k in OPTIONS and "exempt" not in OPTIONS[k], k
        assert any("sweep" in OPTIONS[k] and o[k] in OPTIONS[k]["sweep"] for k in o), (o, "sweeps nothing of the table")
