"""The source condition of the allocation path (tracs_amd/csrc/alloc_path.h): device and pinned memory is allocated and
freed in four functions and nowhere else, and no file keeps a checking macro of its own beside TRACS_HIP_CHECK / TRACS_NCCL_CHECK.
Reads the sources only; needs neither the built library nor a GPU."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tracs_amd", "csrc")
CALLS = ("hipMalloc(", "hipHostMalloc(", "hipFree(", "hipHostFree(")
# the function that may hold each call
HOME = {"hipMalloc(": "device_alloc", "hipHostMalloc(": "pinned_alloc", "hipFree(": "device_free", "hipHostFree(": "pinned_free"}
THE_EXCEPTION = ("capi.hip", "warm_up_body", "hipFree(nullptr)")         # tracs_warm_up's thread: wakes the runtime, frees nothing


def sources():
    files = sorted(f for ext in ("hip", "cpp", "h") for f in glob.glob(os.path.join(CSRC, "*." + ext)))
    assert len(files) > 30 and any(f.endswith("alloc_path.h") for f in files)
    return files


def code_only(text):
    """`text` with comments and the contents of string and character literals blanked, offsets and newlines kept."""
    out = []
    i, n = 0, len(text)
    while i < n:
        c = text[i]
        if text.startswith("//", i):
            j = text.find("\n", i)
            j = n if j < 0 else j
            out.append(" " * (j - i))
            i = j
        elif text.startswith("/*", i):
            j = text.find("*/", i + 2)
            j = n if j < 0 else j + 2
            out.append("".join(ch if ch == "\n" else " " for ch in text[i:j]))
            i = j
        elif c in "\"'":
            j = i + 1
            while j < n and text[j] != c:
                j += 2 if text[j] == "\\" else 1
            out.append(c + " " * (j - i - 1) + c)
            i = j + 1
        else:
            out.append(c)
            i += 1
    return "".join(out)


def enclosing_function(code, pos):
    """The name of the function whose body holds offset `pos`: the identifier in front of the parameter list of the outermost
    brace block around it that follows a ')' (namespaces, extern "C" and structs are passed over)."""
    depth_open = []
    for m in re.finditer(r"[{}]", code[:pos]):
        if m.group() == "{":
            depth_open.append(m.start())
        elif depth_open:
            depth_open.pop()
    for brace in depth_open:                     # outermost first
        head = code[:brace].rstrip()
        head = re.sub(r"(\s*(const|noexcept|override))+$", "", head)
        if not head.endswith(")"):
            continue
        depth, k = 0, len(head) - 1
        while k >= 0:
            depth += head[k] == ")"
            depth -= head[k] == "("
            if depth == 0:
                break
            k -= 1
        name = re.search(r"([A-Za-z_~][\w:~]*)\s*$", head[:k])
        if name and name.group(1) not in ("if", "for", "while", "switch"):
            return name.group(1)
    return None


def test_code_only_and_enclosing_function_on_a_sample():
    sample = 'namespace x {\n// hipFree(a)\nstatic int f(int a) { if (a) { g("hipFree(q)"); hipFree(p); } return 0; }\n}\n'
    code = code_only(sample)
    assert code.count("hipFree(") == 1 and len(code) == len(sample)
    assert enclosing_function(code, code.index("hipFree(")) == "f"


def test_device_and_pinned_memory_is_allocated_and_freed_in_four_functions_only():
    found = {c: 0 for c in CALLS}
    strays = []
    for path in sources():
        code = code_only(open(path).read())
        for call in CALLS:
            for m in re.finditer(r"(?<![\w])" + re.escape(call), code):
                where = enclosing_function(code, m.start())
                line = code.count("\n", 0, m.start()) + 1
                if where == HOME[call] and os.path.basename(path) == "alloc_path.h":
                    found[call] += 1
                elif (os.path.basename(path), where) == THE_EXCEPTION[:2] and code.startswith(THE_EXCEPTION[2], m.start()):
                    found["exception"] = found.get("exception", 0) + 1
                else:
                    strays.append("%s:%d %s in %s" % (os.path.basename(path), line, call, where))
    assert not strays, "\n".join(strays)
    assert all(found[c] == 1 for c in CALLS), found           # each of the four holds its call, once
    assert found.get("exception") == 1                        # tracs_warm_up's hipFree(nullptr), the one named exception


def test_the_only_checking_macros_are_the_two_shared_ones():
    macros = []
    for path in sources():
        for m in re.finditer(r"^[ \t]*#[ \t]*define[ \t]+(\w+_(?:CHECK|TRY))\b", code_only(open(path).read()), re.M):
            macros.append((os.path.basename(path), m.group(1)))
    assert sorted(macros) == [("comm.cpp", "TRACS_NCCL_CHECK"), ("common.h", "TRACS_HIP_CHECK")], macros
