"""The C headers of include/ as the tests read them: the one parser of the library's prototypes and of the C types they are spelled in."""
import ctypes
import os
import re

INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
_VALUE_TYPES = {"int": ctypes.c_int, "long long": ctypes.c_longlong, "float": ctypes.c_float, "size_t": ctypes.c_size_t}


def header_text(*paths):
    """the headers at `paths` (no argument: every include/*.h) without comments, preprocessor lines and the opening of extern "C" """
    paths = paths or [os.path.join(INCLUDE, f) for f in sorted(os.listdir(INCLUDE)) if f.endswith(".h")]
    hdr = "".join(open(p).read() for p in paths)
    hdr = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)                     # comments first: they quote prototypes
    hdr = re.sub(r"//[^\n]*", " ", hdr)
    return re.sub(r"^\s*#[^\n]*$", " ", hdr, flags=re.M).replace('extern "C" {', " ")


def ctype(text, result=False, structs=None):
    """the ctypes type of a C type as the header spells it"""
    t = " ".join(text.replace("*", " * ").split())
    if result and t == "void":
        return None
    if result and t == "const char *":
        return ctypes.c_char_p
    if "*" in t or t == "catseg_stream_t":
        return ctypes.c_void_p
    if structs and t in structs:
        return structs[t]
    return _VALUE_TYPES[t.replace("const ", "")]


def prototypes(*header_file_names):
    """{name: (restype, [argtypes], [argnames])} of every catseg_* prototype of the named headers of include/ (no argument: of every
    include/*.h); a statement that is neither a prototype nor a typedef fails"""
    hdr = header_text(*(os.path.join(INCLUDE, f) for f in header_file_names))
    hdr = re.sub(r"typedef\s+struct\s*\{.*?\}\s*\w+\s*;", " ", hdr, flags=re.S).replace("}", " ")      # (the brace of extern "C")
    protos = {}
    for stmt in hdr.split(";"):
        m = re.match(r"^\s*(?:typedef\b.*|(.+?)\b(catseg_[a-z0-9_]+)\s*\((.*)\))\s*$", stmt, flags=re.S)
        assert m or not stmt.strip(), "cannot parse %r" % stmt
        if m and m.group(2):
            args = [a.strip() for a in m.group(3).split(",")]
            args = [] if args == ["void"] else [re.match(r"^(.*?)(\w+)$", a, flags=re.S).groups() for a in args]
            protos[m.group(2)] = (ctype(m.group(1), result=True), [ctype(t) for t, _ in args], [n for _, n in args])
    return protos
