"""The binding's signature table (_native.SIGNATURES, _native.RESTYPES) against the prototypes of include/psh.h: the same
names, and for each entry point the same number of arguments, each of the header's class -- a pointer, an integer of the
header's width and signedness, or a double -- and the same class of return value.  The compiler holds psh_capi.hip to the
header; this holds the ctypes side to it, where an int for an int64_t works until a value passes 2^31."""
import ctypes as C
import re
from pathlib import Path

import pytest

from shadowing_amd import _native

REPO = Path(__file__).resolve().parent.parent

C_CLASSES = {"int": "i32", "int32_t": "i32", "int64_t": "i64", "uint64_t": "u64", "size_t": "u64", "double": "f64"}


def header_prototypes() -> dict:
    """{name: (return class, [argument classes])} of every function include/psh.h declares."""
    text = (REPO / "include" / "psh.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    text = re.sub(r"^\s*#.*$", "", text, flags=re.M)

    def c_class(decl: str, named: bool) -> str:
        decl = " ".join(decl.replace("*", " * ").split())
        if "*" in decl:
            return "ptr"
        words = [w for w in decl.split() if w != "const"]
        return C_CLASSES[" ".join(words[:-1] if named else words)]

    protos = {}
    for ret, name, args in re.findall(r"([A-Za-z_][\w\s\*]*?)\b(psh_[a-z_0-9]+)\s*\(([^)]*)\)\s*;", text):
        args = [] if args.strip() in ("", "void") else args.split(",")
        protos[name] = (c_class(ret, named=False), [c_class(a, named=True) for a in args])
    return protos


def ctypes_class(t) -> str:
    if t in (C.c_void_p, C.c_char_p) or issubclass(t, C._Pointer):
        return "ptr"
    if t is C.c_double:
        return "f64"
    assert issubclass(t, C._SimpleCData) and t._type_ in "bBhHiIlLqQ", t
    return ("i" if t(-1).value < 0 else "u") + str(8 * C.sizeof(t))


PROTOS = header_prototypes()


def test_the_parser_reads_the_header():
    assert len(PROTOS) >= 50
    assert PROTOS["psh_version"] == ("i32", [])
    assert PROTOS["psh_strerror"] == ("ptr", ["i32"])
    assert PROTOS["psh_embed_plan_offset"] == ("u64", [])
    assert PROTOS["psh_workspace_bytes"] == ("i32", ["i64", "i64", "i32", "i32", "i32", "i32", "ptr"])
    assert PROTOS["psh_mrw_generate"][1][:5] == ["i32", "ptr", "i64", "i32", "f64"] and PROTOS["psh_mrw_generate"][1][8] == "u64"


def test_the_table_names_exactly_the_headers_entry_points():
    assert set(_native.SIGNATURES) == set(PROTOS)
    assert _native.EXPORTS == tuple(_native.SIGNATURES)
    assert set(_native.RESTYPES) <= set(_native.SIGNATURES)


@pytest.mark.parametrize("name", sorted(PROTOS))
def test_signature_matches_the_header(name):
    ret, args = PROTOS[name]
    bound = _native.SIGNATURES[name]
    assert len(bound) == len(args), f"{name}: the header declares {len(args)} arguments, the binding passes {len(bound)}"
    assert [ctypes_class(t) for t in bound] == args
    assert ctypes_class(_native.RESTYPES.get(name, C.c_int)) == ret


def test_load_applies_the_table():
    from shadowing_amd import _build
    _build.build()                       # hipcc cross-compiles gfx950 without a GPU
    lib = _native.load()
    for name, argtypes in _native.SIGNATURES.items():
        fn = getattr(lib, name)
        assert list(fn.argtypes) == list(argtypes) and fn.restype is _native.RESTYPES.get(name, C.c_int), name
