"""The USSEG_* switches are declared once: csrc/knobs.h (kernel library), ultrasound_modeling_amd/knobs.py (Python side), and one table in
DESIGN.md section 4d.  These checks keep the three in step and keep every other file from reading the environment on its own.  The C++
table is read as text (one regular X(...) line per switch); nothing is compiled."""
import glob
import importlib.util
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "ultrasound_modeling_amd")
CSRC = os.path.join(PKG, "csrc")
PER_CALL = {"USSEG_STREAM_MIN_STEPS", "USSEG_STREAM_WGX", "USSEG_STREAM_MERGE", "USSEG_BIG_W8", "USSEG_TCONV_HALO"}
BENCH_HOOKS = {"USSEG_BENCH_FAIL_RANK", "USSEG_BENCH_SHARE_GPU"}      # read by bench.py alone; documented, in neither table


def _read(path):
    with open(path, errors="replace") as f:
        return f.read()


def _py_knobs():
    """knobs.py loaded on its own (it imports nothing but os): no torch, no library."""
    spec = importlib.util.spec_from_file_location("usseg_knobs_table", os.path.join(PKG, "knobs.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _c_rows():
    """[(id, name, kind, default, lifetime)] of csrc/knobs.h; every X( line of the table must parse."""
    text = _read(os.path.join(CSRC, "knobs.h"))
    table = text[text.index("#define USSEG_KNOBS(X)"):text.index("// clang-format on")]
    row = re.compile(r'^\s*X\((K_[A-Z0-9_]+),\s*"(USSEG_[A-Z0-9_]+)",\s*(INT|PRESENT),\s*(-?\d+),\s*(ONCE|PER_CALL),\s*"[^"]+"\)\s*\\?$')
    lines = [ln for ln in table.splitlines()[1:] if ln.strip().startswith("X(")]
    rows = [row.match(ln) for ln in lines]
    assert all(rows), [ln for ln, m in zip(lines, rows) if not m]
    return [(m.group(1), m.group(2), m.group(3), int(m.group(4)), m.group(5)) for m in rows]


def test_only_the_accessors_read_the_environment():
    for path in sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.inc")) + glob.glob(os.path.join(CSRC, "*.h"))):
        if os.path.basename(path) != "knobs.h":
            assert "getenv(" not in _read(path), f"{path}: read the switch through knob<K_...>() (csrc/knobs.h)"
    assert _read(os.path.join(CSRC, "knobs.h")).count("getenv(") == 1
    for path in sorted(glob.glob(os.path.join(PKG, "*.py"))):
        if os.path.basename(path) == "knobs.py":
            continue
        for ln in _read(path).splitlines():
            assert not ("environ" in ln and "USSEG_" in ln.split("#")[0]), f"{path}: read the switch through knobs.get() ({ln.strip()})"
    # ... and every switch the sources name goes through a table entry that exists
    py = _py_knobs().KNOBS
    for path in sorted(glob.glob(os.path.join(PKG, "*.py"))):
        for name in re.findall(r'knobs\.get\("([^"]+)"\)', _read(path)):
            assert name in py, (path, name)
    ids = {r[0] for r in _c_rows()}
    used = set()
    for path in glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.inc")):
        used |= set(re.findall(r"knob<(\w+)>", _read(path)))
    assert used == ids, (used ^ ids)       # no dead table line either


def test_no_name_twice_and_shared_names_agree():
    rows = _c_rows()
    names = [r[1] for r in rows]
    assert len(set(names)) == len(names) and len({r[0] for r in rows}) == len(rows)
    assert all(r[0] == "K_" + r[1][len("USSEG_"):] for r in rows)
    assert all(r[3] == 0 for r in rows if r[2] == "PRESENT")
    src = _read(os.path.join(PKG, "knobs.py"))
    keys = re.findall(r'^\s*"(USSEG_[A-Z0-9_]+)":', src, re.M)
    py = _py_knobs().KNOBS
    assert len(keys) == len(set(keys)) == len(py)           # (a dict literal would swallow a repeated key)
    c = {r[1]: r for r in rows}
    for name in set(c) & set(py):
        assert c[name][2] == "INT" and py[name][0] in ("flag", "int") and py[name][1] == c[name][3], name


def test_per_call_switches_are_exactly_the_five_the_tests_flip():
    assert {r[1] for r in _c_rows() if r[4] == "PER_CALL"} == PER_CALL


def test_tests_and_tools_set_only_declared_switches():
    known = {r[1] for r in _c_rows()} | set(_py_knobs().KNOBS) | BENCH_HOOKS
    name = r"(USSEG_[A-Z0-9_]+)"
    setters = [re.compile(p) for p in (
        r"setenv\(\s*[\"']" + name,                     # monkeypatch.setenv / os.putenv-style calls
        r"environ\[\s*[\"']" + name,                    # os.environ["X"] = ...
        r"[\"']" + name + r"[\"']\s*:",                 # {"X": "1"} handed to a worker as its environment
        r"\b" + name + r"=(?!=)",                       # dict(os.environ, X="1"), env.update(X=...), shell `X=1 cmd`, `export X=...`
    )]
    files = [p for d in ("tests", "tools") for p in glob.glob(os.path.join(ROOT, d, "**", "*"), recursive=True)
             if os.path.isfile(p) and "__pycache__" not in p and os.path.abspath(p) != os.path.abspath(__file__)]
    assert len(files) > 50
    seen, unknown = set(), []
    for path in sorted(files):
        text = _read(path)
        for rx in setters:
            for m in rx.finditer(text):
                seen.add(m.group(1))
                if m.group(1) not in known:
                    unknown.append((os.path.relpath(path, ROOT), m.group(1)))
    assert not unknown, unknown
    assert PER_CALL <= seen and "USSEG_QUAD_HEAD" in seen and "USSEG_LAZY_WGRAD" in seen     # the scan does see setenv, dicts, environ[] and shell forms


def test_design_table_lists_every_switch_with_its_default():
    text = _read(os.path.join(ROOT, "DESIGN.md"))
    table = text[text.index("| Switch | Default | Kind | Read | Read by | What it selects |"):]
    table = table[:table.index("\n\n")]
    doc = {}
    for ln in table.splitlines()[2:]:
        cells = [c.strip() for c in ln.strip().strip("|").split("|")]
        assert len(cells) == 6 and re.fullmatch(r"`USSEG_[A-Z0-9_]+`", cells[0]), ln
        assert cells[0] not in doc, ln
        doc[cells[0].strip("`")] = cells
    py = _py_knobs().KNOBS
    want = {}
    for _, name, kind, default, life in _c_rows():
        want[name] = ("-" if kind == "PRESENT" else str(default), kind, "per call" if life == "PER_CALL" else "once")
    for name, (rule, default, _) in py.items():
        if name not in want:
            want[name] = ("-" if default is None else str(default), rule, "")
    assert set(doc) == set(want) | BENCH_HOOKS, set(doc) ^ (set(want) | BENCH_HOOKS)
    for name, (default, kind, life) in want.items():
        assert doc[name][1] == default, (name, doc[name][1], default)
        assert doc[name][2].split(" / ")[0] == kind, (name, doc[name][2])
        assert doc[name][3].startswith(life), (name, doc[name][3])


def test_python_accessor_defaults_and_parsing(monkeypatch):
    K = _py_knobs()
    for name in list(os.environ):
        if name.startswith("USSEG_"):
            monkeypatch.delenv(name)
    with pytest.raises(KeyError):
        K.get("USSEG_NO_SUCH_SWITCH")
    with pytest.raises(KeyError):
        K.get("USSEG_BIG")             # a switch of the kernel library is not readable from Python
    for name, (rule, default, meaning) in K.KNOBS.items():
        assert rule in ("flag", "int", "optint", "str") and meaning
        got = K.get(name)
        if rule == "flag":
            assert default in (0, 1) and got is bool(default), name
        elif rule == "optint":
            assert default is None and got is None, name
        else:
            assert got == default and (rule == "str" or type(got) is int), name
    # read when called, parsed by the rule
    monkeypatch.setenv("USSEG_QUAD_HEAD", "0")
    assert K.get("USSEG_QUAD_HEAD") is False
    monkeypatch.setenv("USSEG_QUAD_HEAD", "yes")
    assert K.get("USSEG_QUAD_HEAD") is True
    monkeypatch.setenv("USSEG_QUAD_UP", "1")
    assert K.get("USSEG_QUAD_UP") is True
    monkeypatch.setenv("USSEG_ENC_LAZY", "8")
    assert K.get("USSEG_ENC_LAZY") == 8
    monkeypatch.setenv("USSEG_CARD_BWD_MAX_PX", "4096")
    assert K.get("USSEG_CARD_BWD_MAX_PX") == 4096
    monkeypatch.setenv("USSEG_VIT_LAZY", "block")
    assert K.get("USSEG_VIT_LAZY") == "block"
    assert K.get("USSEG_DIST_BACKEND") is None and K.get("USSEG_LIB") is None
