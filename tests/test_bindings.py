"""tracs_amd/_lib.py's signature table against the C declarations: include/tracs_hip.h and tracs_amd/csrc/debug_api.h are parsed
here (the product never parses C) and every prototype is compared with its (restype, argtypes) row, every exported tracs_* symbol
with the table, every struct of the header with its ctypes mirror, and the named constants with the #defines.  The compiler ties
the declarations to the definitions (every defining source includes its header), so a new entry point needs one prototype and one
table row and no test of its own.  CPU only."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from tracs_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PUBLIC_H = os.path.join(ROOT, "include", "tracs_hip.h")
DEBUG_H = os.path.join(ROOT, "tracs_amd", "csrc", "debug_api.h")
N_DEBUG_ONLY = 30                     # the tracs_debug_* entry points debug_api.h declares (three more are in the public header)

# the ctypes mirror of every struct the public header defines with a body
MIRRORS = {"tracs_rules": _lib.Rules, "tracs_tree_request": _lib.TreeRequest, "tracs_tree_result": _lib.TreeResult,
           "tracs_tree_iterate": _lib.TreeIterate, "tracs_tree_iterate_result": _lib.TreeIterateResult}

# C scalar types as the headers spell them -> a ctypes type of that size, signedness and kind on this ABI
C_SCALARS = {"char": C.c_char, "int": C.c_int, "long": C.c_long, "unsigned long long": C.c_ulonglong, "float": C.c_float,
             "double": C.c_double, "size_t": C.c_size_t, "int8_t": C.c_int8, "int16_t": C.c_int16, "int32_t": C.c_int32, "int64_t": C.c_int64,
             "uint8_t": C.c_uint8, "uint16_t": C.c_uint16, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64}


# ---- a small parser for the two headers -----------------------------------------------------------------------------------------

def strip_c(text):
    """comments, preprocessor lines (with their continuations) and the extern "C" brace out of a header"""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    text = re.sub(r"^[ \t]*#(?:[^\n]*\\\n)*[^\n]*$", " ", text, flags=re.M)
    return re.sub(r'extern\s+"C"\s*\{', " ", text)


def parse_type(decl):
    """'const char *const *fasta' -> (('char',), 2, 'const char *const *'): the base type's words, the pointer depth, and the
    spelling without the parameter's name"""
    tokens = re.findall(r"\w+|\*", decl)
    words = [t for t in tokens if t not in ("*", "const")]
    base = tuple(w for w in words if w in C_SCALARS or w in ("void", "unsigned", "signed", "short", "struct") or w.startswith("tracs_"))
    names = [w for w in words if w not in base]
    assert base and len(names) <= 1, "cannot read the C type of %r" % decl
    if names:
        assert tokens[-1] == names[0], "cannot read the C type of %r" % decl
        tokens = tokens[:-1]
    return base, tokens.count("*"), " ".join(tokens).replace("* ", "*").replace("* ", "*")


def parse_header(text):
    """-> ({function: (return type, [argument types])}, {struct: [(field, type)]}), types as parse_type gives them.  Every
    statement of the header must be one of: a prototype, a struct with a body, an opaque struct typedef."""
    text = strip_c(text)
    structs = {}
    for body, name in re.findall(r"typedef\s+struct\s+\w+\s*\{(.*?)\}\s*(\w+)\s*;", text, flags=re.S):
        fields = []
        for stmt in filter(None, (s.strip() for s in body.split(";"))):
            first, *more = stmt.split(",")
            base, depth, spelt = parse_type(first)
            fields.append((re.findall(r"\w+", first)[-1], (base, depth, spelt)))
            for d in more:                                  # `const char *path, *ref`: the base type and its const carry over
                stars = d.count("*")
                head = spelt.split("*")[0].strip()
                fields.append((re.findall(r"\w+", d)[-1], (base, stars, head + (" " + "*" * stars if stars else ""))))
        structs[name] = fields
    text = re.sub(r"typedef\s+struct\s+\w+\s*\{.*?\}\s*\w+\s*;", " ", text, flags=re.S)
    text = re.sub(r"typedef\s+struct\s+\w+\s+\w+\s*;", " ", text)
    protos = {}
    for stmt in (s.strip() for s in text.split(";")):
        if stmt in ("", "}"):
            continue
        m = re.fullmatch(r"(.+?)\b(\w+)\s*\((.*)\)", stmt, flags=re.S)
        assert m, "not a prototype: %r" % stmt
        ret, name, args = m.groups()
        assert name not in protos, name + " is declared twice"
        args = [] if args.strip() == "void" else [parse_type(a) for a in args.split(",")]
        protos[name] = (parse_type(ret), args)
    return protos, structs


def parse_defines(text):
    return {k: int(v) for k, v in re.findall(r"^[ \t]*#define[ \t]+TRACS_(\w+)[ \t]+(-?\d+)\b", text, flags=re.M)}


# ---- the comparison ---------------------------------------------------------------------------------------------------------------

def _kind(t):
    """size, signedness and float-ness of a ctypes scalar"""
    if t in (C.c_float, C.c_double, C.c_longdouble):
        return C.sizeof(t), True, "float"
    if t is C.c_char:
        return 1, True, "int"
    return C.sizeof(t), t(-1).value < 0, "int"


def _is_scalar(t):
    return isinstance(t, type) and issubclass(t, C._SimpleCData) and t not in (C.c_void_p, C.c_char_p, C.c_wchar_p)


def mismatch(ctype, bound, mirrors=MIRRORS):
    """None when the ctypes type `bound` may stand for the C type, else what is wrong"""
    base, depth, spelt = ctype
    cname = " ".join(base)
    if depth == 0:
        if cname == "void":
            return None if bound is None else "void is bound to %r" % (bound,)
        if cname not in C_SCALARS:
            return "%s by value" % cname
        if not _is_scalar(bound):
            return "the scalar %s is bound to %r" % (spelt, bound)
        return None if _kind(bound) == _kind(C_SCALARS[cname]) else "%s is bound to %s" % (spelt, bound.__name__)
    if bound is C.c_void_p:
        return None
    if bound is C.c_char_p:
        return None if (cname, depth) == ("char", 1) else "c_char_p stands for %s" % spelt
    if not (isinstance(bound, type) and issubclass(bound, C._Pointer)):
        return "the pointer %s is bound to %r" % (spelt, bound)
    to = bound._type_
    if to is C.c_char_p:
        return None if spelt == "const char *const *" else "POINTER(c_char_p) stands for %s" % spelt
    if to is C.c_void_p:
        return None if depth >= 2 else "POINTER(c_void_p) stands for %s" % spelt
    if issubclass(to, C.Structure):
        return None if depth == 1 and mirrors.get(cname) is to else "POINTER(%s) stands for %s" % (to.__name__, spelt)
    if depth != 1 or cname not in C_SCALARS or not _is_scalar(to) or _kind(to) != _kind(C_SCALARS[cname]):
        return "POINTER(%s) stands for %s" % (to.__name__, spelt)
    return None


def signature_reports(header_texts, table):
    """every disagreement between the prototypes of the headers and the table, one line each, led by the function's name"""
    protos = {}
    for text in header_texts:
        got = parse_header(text)[0]
        assert not set(got) & set(protos), "declared in both headers: %s" % sorted(set(got) & set(protos))
        protos.update(got)
    out = []
    for name, (ret, args) in sorted(protos.items()):
        if name not in table:
            out.append("%s: declared, but not in the table" % name)
            continue
        restype, argtypes = table[name]
        bad = mismatch(ret, restype)
        if bad:
            out.append("%s: return type: %s" % (name, bad))
        if len(args) != len(argtypes):
            out.append("%s: %d arguments declared, %d bound" % (name, len(args), len(argtypes)))
            continue
        for k, (a, b) in enumerate(zip(args, argtypes)):
            bad = mismatch(a, b)
            if bad:
                out.append("%s: argument %d: %s" % (name, k, bad))
    out += ["%s: in the table, but declared in no header" % name for name in sorted(set(table) - set(protos))]
    return out


def struct_reports(public_text, tmp_path, mirrors=MIRRORS):
    """every disagreement between the structs of the header text and their ctypes mirrors, led by the struct's name: one C program,
    written from the header's own field names, prints every sizeof and offsetof"""
    structs = parse_header(public_text)[1]
    out = ["%s: the header defines it, no ctypes mirror" % s for s in sorted(set(structs) - set(mirrors))]
    out += ["%s: a ctypes mirror, but the header does not define it" % s for s in sorted(set(mirrors) - set(structs))]
    both = sorted(set(structs) & set(mirrors))
    lines = ["#include <stdio.h>", public_text, "int main(void) {"]
    for s in both:
        lines.append('    printf("%s %%zu\\n", sizeof(%s));' % (s, s))
        for f, _ in structs[s]:
            lines.append('    printf("%s.%s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s *)0)->%s));' % (s, f, s, f, s, f))
    lines += ["    return 0;", "}"]
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "no host C compiler"
    exe = os.path.join(str(tmp_path), "layout_%d" % len(os.listdir(str(tmp_path))))
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-x", "c", "-", "-o", exe], input="\n".join(lines), text=True, check=True)
    got = {}
    for line in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines():
        key, *nums = line.split()
        got[key] = [int(x) for x in nums]
    for s in both:
        m = mirrors[s]
        names, mine = [f for f, _ in structs[s]], [f[0] for f in m._fields_]
        if names != mine:
            out.append("%s: fields %s in the header, %s in %s" % (s, names, mine, m.__name__))
            continue
        if got[s] != [C.sizeof(m)]:
            out.append("%s: %d bytes in C, %d in %s" % (s, got[s][0], C.sizeof(m), m.__name__))
        for (f, ctype), (_, bound) in zip(structs[s], m._fields_):
            d = getattr(m, f)
            if got[s + "." + f] != [d.offset, d.size]:
                out.append("%s.%s: offset and size %s in C, %s in %s" % (s, f, got[s + "." + f], [d.offset, d.size], m.__name__))
            bad = mismatch(ctype, bound, mirrors)
            if bad:
                out.append("%s.%s: %s" % (s, f, bad))
    return out


# ---- the tests ------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def headers():
    return open(PUBLIC_H).read(), open(DEBUG_H).read()


def _table():
    return {**_lib.BINDINGS, **_lib.DEBUG_BINDINGS}


def test_the_parser_finds_every_prototype(headers):
    public, debug = (parse_header(t)[0] for t in headers)
    assert sorted(public) == sorted(_lib.SYMBOLS) and len(public) == len(_lib.SYMBOLS) == len(_lib.BINDINGS)
    assert len(debug) == N_DEBUG_ONLY and all(n.startswith("tracs_debug_") for n in debug)
    assert sorted(debug) == sorted(_lib.DEBUG_BINDINGS) and not set(debug) & set(public)
    # counted a second way, so that a prototype the statement parser drops cannot go unnoticed: every `tracs_x(` outside comments
    for text, protos in zip(headers, (public, debug)):
        assert sorted(set(re.findall(r"\b(tracs_\w+)\s*\(", strip_c(text)))) == sorted(protos)


def test_every_prototype_has_its_row_and_every_row_its_prototype(headers):
    assert signature_reports(headers, _table()) == []


def test_every_row_is_complete():
    for name, row in _table().items():
        restype, argtypes = row
        assert isinstance(argtypes, list), name


def test_load_applies_the_table(hiplib):
    for name, (restype, argtypes) in _table().items():
        f = getattr(hiplib, name)
        assert f.restype is restype and list(f.argtypes) == argtypes, name


def test_every_exported_entry_point_is_in_the_table(hiplib):
    nm = shutil.which("nm")
    assert nm, "no nm to read the library's dynamic symbols with"
    out = subprocess.run([nm, "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1].split("@")[0] for line in out.splitlines() if line.strip()}
    exported = {s for s in exported if s.startswith("tracs_")}
    assert len(exported) >= len(_lib.SYMBOLS)
    assert sorted(exported - set(_table())) == [], "exported, but neither declared nor bound"
    assert sorted(set(_table()) - exported) == [], "in the table, but not exported"


def test_the_struct_mirrors_have_the_header_s_layout(headers, tmp_path):
    assert len(parse_header(headers[0])[1]) == len(MIRRORS) == 5 and parse_header(headers[1])[1] == {}
    assert struct_reports(headers[0], tmp_path) == []


def test_the_named_constants_are_the_header_s(headers):
    defines = parse_defines(headers[0])
    codes = {k: v for k, v in defines.items() if k.startswith("E_")}
    assert sorted(codes, key=lambda k: -codes[k]) == ["E_ARG", "E_FASTA", "E_RAGGED", "E_OPEN", "E_HIP", "E_NOMEM", "E_INTERRUPTED"]
    for name, value in dict(codes, TREE_BIONJ=defines["TREE_BIONJ"]).items():
        assert getattr(_lib, name) == value, name


def _edit(text, old, new):
    assert text.count(old) == 1, old
    return text.replace(old, new)


DOCTORED_PROTOTYPES = [
    # (function, header, the text of its prototype, the doctored text)
    ("tracs_nj_init", 0, "int tracs_nj_init(void *state, size_t n, void *stream);", "int tracs_nj_init(void *state, void *stream);"),
    ("tracs_nj_run", 0, "int tracs_nj_run(void *state, size_t n, void *stream);", "int tracs_nj_run(void *state, int n, void *stream);"),
    ("tracs_bootstrap_weights", 0, "int tracs_bootstrap_weights(size_t L, uint64_t seed,", "int tracs_bootstrap_weights(size_t L, double seed,"),
    ("tracs_edges_count_f64", 0, "int32_t dist_threshold, double threshold, int64_t *offsets, void *stream);",
     "int32_t dist_threshold, uint64_t threshold, int64_t *offsets, void *stream);"),
    ("tracs_msf_init", 0, "int tracs_msf_init(void *state, size_t n, void *stream);", "int tracs_msf_init(size_t state, size_t n, void *stream);"),
    ("tracs_hist_init", 0, "int tracs_hist_init(void *state, size_t n_bins, void *stream);", "int tracs_hist_init(void *state, size_t *n_bins, void *stream);"),
    ("tracs_comm_rank", 0, "int tracs_comm_rank(const tracs_comm *c);", "size_t tracs_comm_rank(const tracs_comm *c);"),
    ("tracs_pairsnp_free", 0, "void tracs_pairsnp_free(tracs_pairsnp_result *r);", "int tracs_pairsnp_free(tracs_pairsnp_result *r);"),
    ("tracs_distance_tree_run", 0, "const tracs_tree_request *req, tracs_tree_result *res);", "const tracs_tree_iterate *req, tracs_tree_result *res);"),
    ("tracs_alignment_select_samples", 0, "const uint8_t *keep_sample, tracs_alignment **out, void *stream);", "const int8_t *keep_sample, tracs_alignment **out, void *stream);"),
    ("tracs_debug_pack_stages", 1, "int tracs_debug_pack_stages(char *names, size_t cap, float *ms,", "int tracs_debug_pack_stages(char *names, size_t cap, double *ms,"),
    ("tracs_debug_format_floats", 1, "long tracs_debug_format_floats(const double *x, size_t n, char *buf,", "long tracs_debug_format_floats(const double *x, size_t n, uint8_t *buf,"),
    ("tracs_debug_last_trans_dist_keys", 1, "unsigned long long tracs_debug_last_trans_dist_keys(void);", "unsigned long long tracs_debug_last_trans_dist_keys(int which);"),
]


@pytest.mark.parametrize("name, which, old, new", DOCTORED_PROTOTYPES, ids=["%s-%d" % (d[0], k) for k, d in enumerate(DOCTORED_PROTOTYPES)])
def test_a_doctored_prototype_is_reported_by_name(headers, name, which, old, new):
    """an argument dropped, size_t -> int, uint64_t -> double and double -> uint64_t, a pointer -> a scalar and back, int -> size_t and
    void -> int returns, another struct, another signedness or kind behind a pointer, c_char_p for bytes, an argument added"""
    texts = list(headers)
    texts[which] = _edit(texts[which], old, new)
    reports = signature_reports(texts, _table())
    assert len(reports) == 1 and reports[0].startswith(name + ": "), reports


def test_a_dropped_declaration_and_a_dropped_row_are_reported(headers):
    texts = [headers[0], _edit(headers[1], "int tracs_debug_iupac_mask(int ch);", "")]
    assert signature_reports(texts, _table()) == ["tracs_debug_iupac_mask: in the table, but declared in no header"]
    table = _table()
    del table["tracs_free"]
    assert signature_reports(headers, table) == ["tracs_free: declared, but not in the table"]


DOCTORED_STRUCTS = [
    ("tracs_rules", "    double max_n_share;\n", ""),                                                             # a field removed
    ("tracs_tree_request", "    uint32_t replicates;               /* 0: no bootstrap */\n    uint64_t seed;\n",
     "    uint64_t seed;\n    uint32_t replicates;\n"),                                                          # 4 and 8 bytes swapped
    ("tracs_tree_iterate_result", "    uint32_t iterations;\n    int32_t same_as;\n", "    int32_t iterations;\n    uint32_t same_as;\n"),
    ("tracs_tree_iterate", "    uint32_t max_iterations;\n", "    uint64_t max_iterations;\n"),
]


@pytest.mark.parametrize("name, old, new", DOCTORED_STRUCTS, ids=["%s-%d" % (d[0], k) for k, d in enumerate(DOCTORED_STRUCTS)])
def test_a_doctored_struct_is_reported_by_name(headers, tmp_path, name, old, new):
    """a field removed, two adjacent fields of different size swapped, two signednesses swapped (same layout), a field widened"""
    reports = struct_reports(_edit(headers[0], old, new), tmp_path)
    assert reports and all(r.startswith(name) for r in reports), reports
