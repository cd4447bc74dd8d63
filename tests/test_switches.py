"""The engine's switches (environment variables) in one place: `read_switches` in csrc/bmo_engine.hip is the only reader under csrc/,
DESIGN.md §3 "Switches" has one row per name it reads, and every BMO_* name a test or a tool hands to the engine through the
environment is one that something reads.  A search over the project's own host sources; no device, no build."""
import ast
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "beamletoptics.jl_amd", "csrc")
NAME = r"BMO_[A-Z0-9_]+"


def _read(path):
    with open(path, encoding="utf-8") as f:
        return f.read()


def _reader():
    """(start, end) of read_switches in bmo_engine.hip, (0, 0) if there is none, and the file's text"""
    text = _read(os.path.join(CSRC, "bmo_engine.hip"))
    m = re.search(r"^Switches read_switches\(\) \{\n.*?^\}\n", text, re.S | re.M)
    return (m.start(), m.end(), text) if m else (0, 0, text)


def _reader_names():
    """the names read_switches reads: every quoted BMO_* name in it (its helpers take the name as their first argument)"""
    a, b, text = _reader()
    return set(re.findall(r'"(%s)"' % NAME, text[a:b]))


def test_one_reader_of_the_environment():
    a, b, _ = _reader()
    stray = []
    for path in sorted(glob.glob(os.path.join(CSRC, "*"))):
        if not os.path.isfile(path) or path.endswith(".so"):
            continue
        for m in re.finditer(r"getenv", _read(path)):
            if not (path.endswith("bmo_engine.hip") and a <= m.start() < b):
                stray.append("%s, offset %d" % (os.path.basename(path), m.start()))
    assert not stray, "getenv outside read_switches: " + "; ".join(stray)
    assert _reader_names(), "read_switches reads nothing"


def test_design_table_lists_what_the_reader_reads():
    design = _read(os.path.join(ROOT, "DESIGN.md"))
    m = re.search(r"^### Switches[^\n]*\n(.*?)^#{2,3} ", design, re.S | re.M)
    assert m, "DESIGN.md has no '### Switches' section"
    rows = re.findall(r"^\| `(%s)` \|" % NAME, m.group(1), re.M)
    assert len(rows) == len(set(rows)), "a switch has two rows"
    assert set(rows) == _reader_names(), sorted(set(rows) ^ _reader_names())


def _handed_by_python(path):
    """BMO_* names a Python file puts into an environment: setenv / delenv calls, os.environ[...] = ..., keys of dict literals, keyword arguments."""
    out = set()
    for node in ast.walk(ast.parse(_read(path), path)):
        names = []
        if isinstance(node, ast.Call):
            names += [k.arg for k in node.keywords if k.arg]
            if isinstance(node.func, ast.Attribute) and node.func.attr in ("setenv", "delenv") and node.args:
                names.append(node.args[0])
        elif isinstance(node, ast.Subscript) and isinstance(node.ctx, ast.Store) and "environ" in ast.dump(node.value):
            names.append(node.slice)
        elif isinstance(node, ast.Dict):
            names += node.keys
        for n in names:
            n = n.value if isinstance(n, ast.Constant) else n
            if isinstance(n, str) and re.fullmatch(NAME, n):
                out.add(n)
    return out


def _handed_by_shell(path):
    """NAME=value words of a shell script outside its comments (a name behind -D is a compile-time macro)"""
    code = "\n".join(line for line in _read(path).splitlines() if not line.lstrip().startswith("#"))
    return set(re.findall(r"(?<![\w-])(%s)=" % NAME, code))


def _read_by_python():
    """names a .py file of the package or the tools reads from os.environ; and bench.py, which tests/test_multi_gpu.py starts as a child
    with BMO_BENCH_FORCE_DIST in its environment: the benchmark reads that one itself, the engine never sees it"""
    files = glob.glob(os.path.join(ROOT, "beamletoptics.jl_amd", "*.py")) + glob.glob(os.path.join(ROOT, "tools", "*.py")) + [os.path.join(ROOT, "bench.py")]
    out = set()
    for path in files:
        out |= set(re.findall(r"""environ(?:\.get|\.pop|\.setdefault)?\s*[\[(]\s*["'](%s)["']""" % NAME, _read(path)))
        out |= set(re.findall(r"""["'](%s)["']\s+(?:not\s+)?in\s+os\.environ""" % NAME, _read(path)))
    return out


def test_every_switch_a_test_or_tool_sets_is_read():
    handed = {}
    for path in sorted(glob.glob(os.path.join(ROOT, "tests", "*.py")) + glob.glob(os.path.join(ROOT, "tools", "*"))):
        if path.endswith(".py"):
            names = _handed_by_python(path)
        elif path.endswith(".sh"):
            names = _handed_by_shell(path)
        else:
            continue
        for n in names:
            handed.setdefault(n, []).append(os.path.relpath(path, ROOT))
    assert {"BMO_DEBUG", "BMO_FUSE", "BMO_ROOT_ORDER", "BMO_WIDE_MIN_WAVES"} <= set(handed), sorted(handed)  # (the search finds the known ones)
    read = _reader_names() | _read_by_python()
    unread = {n: where for n, where in handed.items() if n not in read}
    assert not unread, "set for the engine, read by nothing: %r" % unread
