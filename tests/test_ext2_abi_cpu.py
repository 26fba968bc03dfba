"""CPU: the open extension header include/gngf_ext2.h, held to the discipline tests/test_ext_abi_cpu.py holds include/gngf_ext.h to:
the library exports what the header declares, the binding (_lib.EXT2_SIGNATURES) mirrors it in names, arity and argument kinds,
the version of header, library and binding agree, the three tables share no name, and every entry point either has a guard-band
case in a GPU test file or is listed here as writing no device memory, with the reason.

Unlike the two closed headers this one may grow: nothing here fixes the set of names or the value of the version.  A change that
adds an entry point adds it to the header, to _lib.EXT2_SIGNATURES and to GUARDED_IN or WRITES_NOTHING below, and raises the
version in header and binding together."""
import ctypes
import importlib
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WRITES_NOTHING = {
    "gngf_ext2_version": "returns a constant",
    "gngf_ext2_render_score_workspace_words": "returns a constant",
}
# test module -> the function of it that runs the guard-band cases of the names its entry_points() lists
GUARDED_IN = {
    "test_gpu_score": "test_render_score_guarded",
}


def header_source():
    with open(os.path.join(ROOT, "include", "gngf_ext2.h")) as f:
        return re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)


def header_functions():
    out = {}
    for m in re.finditer(r"\b(?:int|int64_t)\s+(gngf_\w+)\s*\(([^)]*)\)\s*;", header_source()):
        out[m.group(1)] = [" ".join(a.split()) for a in m.group(2).split(",") if a.strip() and a.strip() != "void"]
    return out


def test_library_exports_every_declared_symbol_and_the_versions_agree():
    from collision_handling_in_instantngp_amd import _lib
    lib = _lib.load()
    decl = header_functions()
    assert "gngf_ext2_version" in decl and len(decl) >= 2
    for name in decl:
        assert hasattr(lib, name), f"{name} declared in include/gngf_ext2.h but not exported"
    in_header = int(re.search(r"#define\s+GNGF_EXT2_VERSION\s+(\d+)", header_source()).group(1))
    assert in_header == lib.gngf_ext2_version() == _lib.EXT2_VERSION >= 1


def test_bindings_mirror_header_arity_and_kinds():
    from collision_handling_in_instantngp_amd import _lib
    decl = header_functions()
    assert set(decl) == set(_lib.EXT2_SIGNATURES), set(decl) ^ set(_lib.EXT2_SIGNATURES)
    assert all(name.startswith("gngf_ext2_") for name in decl)
    for name, args in decl.items():
        sig = _lib.EXT2_SIGNATURES[name]
        assert len(sig) == len(args), (name, len(sig), len(args))
        for a, ct in zip(args, sig):
            if "*" in a:
                want = ctypes.c_void_p
            elif a.startswith("int64_t"):
                want = ctypes.c_int64
            elif a.startswith("float") or a.startswith("double"):
                want = ctypes.c_float if a.startswith("float") else ctypes.c_double
            else:
                want = ctypes.c_int
            assert ct is want, (name, a, ct)
    lib = _lib.load()
    for name, sig in _lib.EXT2_SIGNATURES.items():             # bound in load(), next to the other two tables
        assert list(getattr(lib, name).argtypes or []) == list(sig) and getattr(lib, name).restype is ctypes.c_int, name


def test_the_three_tables_are_disjoint_and_the_closed_headers_untouched():
    from collision_handling_in_instantngp_amd import _lib
    tables = [set(_lib.SIGNATURES), set(_lib.EXT_SIGNATURES), set(_lib.EXT2_SIGNATURES)]
    for i in range(3):
        for j in range(i + 1, 3):
            assert not tables[i] & tables[j], sorted(tables[i] & tables[j])
    assert not any(n.startswith("gngf_ext2_") for n in tables[0] | tables[1])
    for closed in ("gngf.h", "gngf_ext.h"):
        with open(os.path.join(ROOT, "include", closed)) as f:
            assert "gngf_ext2_" not in f.read(), closed
    lib = _lib.load()
    assert lib.gngf_abi_version() == _lib.ABI_VERSION and lib.gngf_ext_version() == _lib.EXT_VERSION


def test_call_and_query_serve_all_three_tables():
    from collision_handling_in_instantngp_amd import _lib
    assert _lib.query("gngf_ext2_version") == _lib.EXT2_VERSION
    assert _lib.query("gngf_ext_version") == _lib.EXT_VERSION and _lib.query("gngf_abi_version") == _lib.ABI_VERSION
    words = _lib.query("gngf_ext2_render_score_workspace_words")
    assert words >= 2 and words % 2 == 0                      # a pair of sums per workgroup
    with pytest.raises(RuntimeError, match="hipErrorInvalidValue"):      # all NULL / zero: rejected before any launch
        _lib.call("gngf_ext2_render_score", *[(None if t is ctypes.c_void_p else 0)
                                              for t in _lib.EXT2_SIGNATURES["gngf_ext2_render_score"]])
    _lib.call("gngf_ext_sample_pixels", None, 4, 4, 3, 3.0, 0, None, 0, None, None, 0, None)     # the older table still answers


def test_every_entry_point_has_a_guarded_case_or_a_reason():
    from collision_handling_in_instantngp_amd import _lib
    names = set(_lib.EXT2_SIGNATURES)
    covered = set()
    for module, function in GUARDED_IN.items():
        listed = set(importlib.import_module(module).entry_points())
        assert listed and listed <= names, (module, sorted(listed - names))
        covered |= listed
        # the cases it counts are guard-band cases: the test that runs them checks the arena and what was and was not written
        with open(os.path.join(ROOT, "tests", module + ".py")) as f:
            body = f.read().split(f"def {function}(")[1].split("\ndef ")[0]
        assert "arena.check()" in body and "unwritten" in body, module
    assert set(WRITES_NOTHING) <= names
    missing = names - covered - set(WRITES_NOTHING)
    assert not missing, f"no guard-band case and no reason for: {sorted(missing)}"
    assert not covered & set(WRITES_NOTHING), sorted(covered & set(WRITES_NOTHING))
    assert all(isinstance(why, str) and why.strip() for why in WRITES_NOTHING.values())


def test_entry_points_listed_as_writing_nothing_take_no_writable_pointer():
    decl = header_functions()
    for name in WRITES_NOTHING:
        for param in decl[name]:
            assert "*" not in param or param.startswith("const "), f"{name} takes a writable pointer: {param}"
