"""The run-time switches: tracs_amd/csrc/switches.h and tracs_amd/switches.py each hold one table, and these checks
hold the tables to the code (nothing else reads the environment; every row has a reader of its kind), to DESIGN.md 8 (the same names,
the same lifetimes) and to the tests (a TRACS_* name a test puts in a string is a switch, a constant of the headers, or one of the
harness's few names: a misspelt switch would test the default route and pass).  The checks are functions over texts, run over the tree
and over doctored texts that show each slip reported by name.  Reads the sources only; needs neither the built library nor a GPU."""
import glob
import io
import os
import re
import tokenize

from test_csrc_alloc import code_only

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tracs_amd", "csrc")
KINDS = ("flag", "zero_off", "integer", "real", "size", "text")
# the accessor that reads each kind (is_set besides: whether a variable is there can be asked of any kind)
READER = {"flag": "is_set", "zero_off": "is_zero", "integer": "integer", "real": "real", "size": "size", "text": "text"}
NAME = r"TRACS_[A-Z0-9_]+"

# TRACS_* names in the tests' strings that are no library switch and no constant of the two headers
HARNESS = {
    "TRACS_KEY_SPLIT": "bench.py's own switch (DESIGN.md 5)",
    "TRACS_TEST_POISON": "tests/scratch_poison.py's message to the child processes it poisons",
    "TRACS_REPORT_DIR": "tests/test_gpu_transcluster_hp.py: where its figures also go as JSON",
    "TRACS_REFERENCE": "tests/golden/make_threshold_golden.py: where the reference lies when a golden file is remade",
    "TRACS_HIP_LIB": "INTEGRATION.md's loader snippet, run by tests/test_integration_stub.py",
    "TRACS_HIP_CHECK": "a macro of csrc/common.h, named by tests/test_csrc_alloc.py",
    "TRACS_NCCL_CHECK": "a macro of csrc/comm.cpp, named by tests/test_csrc_alloc.py",
}
HARNESS_PREFIX = "TRACS_BENCH_"          # bench.py's own variables: DESIGN.md 8 keeps their short row


def read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def csrc_texts():
    files = sorted(f for ext in ("hip", "cpp", "h") for f in glob.glob(os.path.join(CSRC, "*." + ext)))
    assert len(files) > 30
    return {os.path.basename(f): open(f).read() for f in files}


def py_texts():
    files = sorted(glob.glob(os.path.join(ROOT, "tracs_amd", "*.py")))
    assert len(files) > 10
    return {os.path.basename(f): open(f).read() for f in files}


def test_texts():
    files = sorted(f for f in glob.glob(os.path.join(ROOT, "tests", "*.py")) if os.path.abspath(f) != os.path.abspath(__file__))
    assert len(files) > 40
    return {os.path.basename(f): open(f).read() for f in files}


test_texts.__test__ = False


# ---- the checks, as functions over texts: each returns its slips, every one with the name it is about ---------------------------------

def c_table(header):
    """{name: (kind, lifetime, effect)} of the rows of switches.h"""
    rows = re.findall(r'^\s*X\((%s),\s*(\w+),\s*(\w+),\s*"([^"]*)"\)' % NAME, header, re.M)
    assert len({r[0] for r in rows}) == len(rows), "a name has two rows"
    return {n: (k, life, effect) for n, k, life, effect in rows}


def stray_getenv(sources):
    """getenv outside switches.h: 'file:line: <the line>'"""
    slips = []
    for name, text in sources.items():
        if name == "switches.h":
            continue
        code = code_only(text)
        for m in re.finditer(r"\bgetenv\b", code):
            line = code.count("\n", 0, m.start())
            slips.append("%s:%d: %s" % (name, line + 1, text.split("\n")[line].strip()))
    return slips


def stray_environ(sources):
    """os.environ / os.getenv reads of a TRACS_* name (or HIPCC) outside switches.py"""
    slips = []
    for name, text in sources.items():
        if name == "switches.py":
            continue
        for m in re.finditer(r"""os\.(?:environ\s*(?:\.get\(|\[)|getenv\()\s*["'](%s|HIPCC)["']""" % NAME, text):
            slips.append("%s:%d: %s" % (name, text.count("\n", 0, m.start()) + 1, m.group(1)))
    return slips


def c_reader_slips(table, sources):
    """rows that no accessor call names, and calls whose accessor is not the one of the row's kind"""
    slips, seen = [], set()
    for name, text in sources.items():
        if name == "switches.h":
            continue
        for m in re.finditer(r"\bsw::(is_set|is_zero|integer|real|size|text)\(\s*(?:tracs::)?sw::(%s)\b" % NAME, code_only(text)):
            how, var = m.groups()
            seen.add(var)
            if var in table and how not in ("is_set", READER[table[var][0]]):
                slips.append("%s: %s: a %s row read with %s()" % (name, var, table[var][0], how))
    return slips + ["%s: no accessor call names it" % v for v in sorted(set(table) - seen)]


def py_reader_slips(table, sources):
    """rows that no switches.get() names (rccl.backend_choice hands the name it is given to get: its callers count, bench.py among them)"""
    seen = set()
    for text in sources.values():
        seen |= set(re.findall(r"""switches\.get\(\s*["'](\w+)["']""", text))
        seen |= set(re.findall(r"""backend_choice\([^()]*["'](\w+)["']\s*\)""", text))
    return ["%s: no switches.get() names it" % v for v in sorted(set(table) - seen)]


def section8(design):
    """{name: lifetime cell} of the variables in the first column of the table of DESIGN.md 8 (bench.py's own and -D flags left out)"""
    body = re.search(r"^## 8\. [^\n]*\n(.*?)(?=^## |\Z)", design, re.M | re.S).group(1)
    out = {}
    for line in body.split("\n"):
        cells = [c.strip() for c in re.split(r"(?<!\\)\|", line)]
        if len(cells) < 5 or set(cells[1]) <= set("-") or cells[1] == "Variable":
            continue
        for m in re.finditer(r"`(-D)?(%s|HIPCC)\b[^`]*`" % NAME, cells[1]):
            if not m.group(1) and not m.group(2).startswith(HARNESS_PREFIX):
                assert m.group(2) not in out, "DESIGN.md 8 has two rows for " + m.group(2)
                out[m.group(2)] = cells[2]
    return out


def section8_slips(ctab, pytab, design):
    doc = section8(design)
    tables = {n for n in set(ctab) | set(pytab) if not n.startswith(HARNESS_PREFIX)}
    slips = ["%s: in a table, no row in DESIGN.md 8" % n for n in sorted(tables - set(doc))]
    slips += ["%s: in DESIGN.md 8, in no table" % n for n in sorted(set(doc) - tables)]
    slips += ["%s: %s in switches.h, '%s' in DESIGN.md 8" % (n, ctab[n][1], doc[n]) for n in sorted(set(ctab) & set(doc)) if doc[n] != ctab[n][1]]
    return slips


def header_names(*headers):
    return set(re.findall(r"\b%s\b" % NAME, "\n".join(code_only(h) for h in headers)))


def names_in(source):
    """the TRACS_* names in the string literals of a Python source (docstrings and the literal parts of f-strings among them), and
    those written as keyword arguments: dict(os.environ, TRACS_X="1")"""
    kinds = {tokenize.STRING, getattr(tokenize, "FSTRING_MIDDLE", tokenize.STRING)}
    toks = list(tokenize.generate_tokens(io.StringIO(source).readline))
    found = {v for t in toks if t.type in kinds for v in re.findall(r"\b%s\b" % NAME, t.string)}
    return found | {t.string for t, nxt in zip(toks, toks[1:]) if t.type == tokenize.NAME and re.fullmatch(NAME, t.string) and nxt.string == "="}


def unknown_test_names(known, sources):
    slips = []
    for name, text in sources.items():
        for var in sorted(names_in(text)):
            if var not in known and var not in HARNESS and not var.startswith(HARNESS_PREFIX):
                slips.append("%s: %s is no switch, no constant of the headers and no name of the harness" % (name, var))
    return slips


# ---- the tree -------------------------------------------------------------------------------------------------------------------------

def tables():
    from tracs_amd import switches
    return c_table(read("tracs_amd", "csrc", "switches.h")), dict(switches.TABLE)


def test_the_tables_are_well_formed():
    ctab, pytab = tables()
    assert len(ctab) >= 40 and len(pytab) >= 8
    assert read("tracs_amd", "csrc", "switches.h").count("    X(TRACS_") == len(ctab)               # the regular expression saw every row
    for n, (kind, life, effect) in ctab.items():
        assert kind in KINDS and life in ("once", "every") and effect, n
    for n, (kind, effect) in pytab.items():
        assert kind in ("flag", "nonempty", "text") and effect, n
    assert "hip" not in re.findall(r'#include [<"]([^>"]*)', read("tracs_amd", "csrc", "switches.h").lower())   # host only


def test_nothing_reads_the_environment_beside_the_two_tables():
    assert not stray_getenv(csrc_texts())
    assert not stray_environ(py_texts())


def test_every_row_has_a_reader_of_its_kind():
    ctab, pytab = tables()
    assert not c_reader_slips(ctab, csrc_texts())
    assert not py_reader_slips(pytab, dict(py_texts(), **{"bench.py": read("bench.py")}))


def test_design_section_8_has_the_tables_rows_and_lifetimes():
    ctab, pytab = tables()
    assert not section8_slips(ctab, pytab, read("DESIGN.md"))


def test_every_name_in_the_tests_strings_is_known():
    ctab, pytab = tables()
    known = set(ctab) | set(pytab) | header_names(read("include", "tracs_hip.h"), read("tracs_amd", "csrc", "debug_api.h"))
    assert "TRACS_TREE_BIONJ" in known and "TRACS_OK" in known
    assert not unknown_test_names(known, test_texts())
    used = {v for text in test_texts().values() for v in names_in(text)}
    assert set(HARNESS) - {"TRACS_KEY_SPLIT", "TRACS_REFERENCE"} <= used          # no allowance outlives its use (those two: bench.py's, tests/golden's)


# ---- doctored texts: each slip is reported, with its name -------------------------------------------------------------------------------

HEADER = '#define TRACS_SWITCHES(X) \\\n    X(TRACS_A, integer, once, "a") \\\n    X(TRACS_B, flag, every, "b")\n'
SOURCE = "int f() { return sw::integer(sw::TRACS_A, -1) + sw::is_set(sw::TRACS_B) + sw::is_set(sw::TRACS_A); }\n"
DESIGN = "## 7. x\n| `TRACS_OLD` | once | no |\n## 8. Switches\n\n| Variable | Lifetime | Effect |\n|---|---|---|\n" \
         "| `TRACS_A=0\\|1` | once | a (`TRACS_NOT_FIRST_COLUMN`) |\n| `TRACS_B=1`, `HIPCC` | every | b, with `-DTRACS_FLAG` |\n" \
         "| `TRACS_BENCH_X`, `-DTRACS_Y=…` | — | bench |\n"


def test_the_doctored_texts_pass_as_they_stand():
    tab = c_table(HEADER)
    assert tab == {"TRACS_A": ("integer", "once", "a"), "TRACS_B": ("flag", "every", "b")}
    assert not stray_getenv({"a.hip": SOURCE, "switches.h": "std::getenv(r.name)"}) and not c_reader_slips(tab, {"a.hip": SOURCE})
    assert section8(DESIGN) == {"TRACS_A": "once", "TRACS_B": "every", "HIPCC": "every"}
    assert not section8_slips(tab, {"HIPCC": ("text", "c"), "TRACS_BENCH_BACKEND": ("text", "d")}, DESIGN)


def test_a_stray_getenv_is_reported():
    slips = stray_getenv({"a.hip": SOURCE + '// getenv("TRACS_IN_A_COMMENT")\nstatic int x = atoi(std::getenv("TRACS_X"));\n'})
    assert len(slips) == 1 and slips[0].startswith("a.hip:3:") and "TRACS_X" in slips[0]
    slips = stray_environ({"a.py": 'v = os.environ.get("TRACS_Y", "1")\nw = os.environ["HIPCC"]\nos.environ["RANK"]\n', "switches.py": 'os.environ.get("TRACS_Z")'})
    assert slips == ["a.py:1: TRACS_Y", "a.py:2: HIPCC"]


def test_a_row_without_a_reader_is_reported_and_so_is_a_reader_of_another_kind():
    tab = c_table(HEADER + '    X(TRACS_DEAD, size, every, "nobody reads it")\n')
    assert c_reader_slips(tab, {"a.hip": SOURCE + '// sw::size(sw::TRACS_DEAD, 0)\n'}) == ["TRACS_DEAD: no accessor call names it"]
    assert c_reader_slips(c_table(HEADER), {"a.hip": SOURCE.replace("sw::integer(", "sw::real(")}) == ["a.hip: TRACS_A: a integer row read with real()"]
    assert py_reader_slips({"TRACS_P": 0, "TRACS_Q": 0, "TRACS_R": 0}, {"a.py": 'switches.get("TRACS_P", "x")\nbackend_choice(w, n, "TRACS_R")\n'}) == \
        ["TRACS_Q: no switches.get() names it"]


def test_a_missing_row_of_section_8_is_reported_both_ways():
    tab = c_table(HEADER)
    assert section8_slips(tab, {}, DESIGN.replace("`TRACS_B=1`, ", "")) == ["TRACS_B: in a table, no row in DESIGN.md 8", "HIPCC: in DESIGN.md 8, in no table"]


def test_a_wrong_lifetime_in_section_8_is_reported():
    slips = section8_slips(c_table(HEADER), {"HIPCC": 0}, DESIGN.replace("| every | b", "| once | b"))
    assert slips == ["TRACS_B: every in switches.h, 'once' in DESIGN.md 8"]


def test_a_misspelt_switch_in_a_test_is_reported():
    text = 'def test_x():\n    """TRACS_FILTER_KERNEL=1"""\n    env = dict(os.environ, TRACS_FILTER_KERNAL="1")\n    run(env={"TRACS_FILTER_KERNAL": "1", ' \
           '"TRACS_BENCH_VERIFY": "0", "TRACS_TEST_POISON": "7"}, rc=L.TRACS_AN_ATTRIBUTE)\n    assert rc == "TRACS_E_ARG"\n'
    slips = unknown_test_names({"TRACS_FILTER_KERNEL", "TRACS_E_ARG"}, {"test_x.py": text})
    assert len(slips) == 1 and slips[0].startswith("test_x.py: TRACS_FILTER_KERNAL ")
