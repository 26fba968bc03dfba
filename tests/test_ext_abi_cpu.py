"""CPU: the extension header include/gngf_ext.h, held to the discipline tests/test_abi.py and tests/test_store_bounds_ledger_cpu.py
hold include/gngf.h to: the library exports what the header declares, the binding (_lib.EXT_SIGNATURES) mirrors it in names, arity
and argument kinds, the exported version is the binding's, and every entry point either has a guard-band case in
tests/test_gpu_sampler.py or is listed here as writing no device memory, with the reason.  include/gngf.h itself stays closed."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WRITES_NOTHING = {
    "gngf_ext_version": "returns a constant",
}


def header_source():
    with open(os.path.join(ROOT, "include", "gngf_ext.h")) as f:
        return re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)


def header_functions():
    out = {}
    for m in re.finditer(r"\b(?:int|int64_t)\s+(gngf_\w+)\s*\(([^)]*)\)\s*;", header_source()):
        out[m.group(1)] = [" ".join(a.split()) for a in m.group(2).split(",") if a.strip() and a.strip() != "void"]
    return out


def test_library_exports_every_declared_symbol_and_its_version():
    from collision_handling_in_instantngp_amd import _lib
    lib = _lib.load()
    decl = header_functions()
    assert set(decl) == {"gngf_ext_version", "gngf_ext_sample_pixels"}
    for name in decl:
        assert hasattr(lib, name), f"{name} declared in include/gngf_ext.h but not exported"
    assert lib.gngf_ext_version() == _lib.EXT_VERSION == 1
    assert int(re.search(r"#define\s+GNGF_EXT_VERSION\s+(\d+)", header_source()).group(1)) == _lib.EXT_VERSION


def test_bindings_mirror_header_arity_and_kinds():
    from collision_handling_in_instantngp_amd import _lib
    decl = header_functions()
    assert set(decl) == set(_lib.EXT_SIGNATURES), set(decl) ^ set(_lib.EXT_SIGNATURES)
    assert all(name.startswith("gngf_ext_") for name in decl)
    for name, args in decl.items():
        sig = _lib.EXT_SIGNATURES[name]
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
    for name, sig in _lib.EXT_SIGNATURES.items():              # bound in load(), next to the closed table
        assert list(getattr(lib, name).argtypes or []) == list(sig) and getattr(lib, name).restype is ctypes.c_int, name


def test_the_closed_abi_is_untouched():
    from collision_handling_in_instantngp_amd import _lib
    assert _lib.ABI_VERSION == 15
    assert not set(_lib.EXT_SIGNATURES) & set(_lib.SIGNATURES)
    with open(os.path.join(ROOT, "include", "gngf.h")) as f:
        assert "gngf_ext_" not in f.read()


def test_call_and_query_serve_both_tables():
    from collision_handling_in_instantngp_amd import _lib
    assert _lib.query("gngf_ext_version") == 1 and _lib.query("gngf_abi_version") == 15
    _lib.call("gngf_ext_sample_pixels", None, 4, 4, 3, 3.0, 0, None, 0, None, None, 0, None)     # P == 0: success, no launch
    with pytest.raises(RuntimeError, match="hipErrorInvalidValue"):
        _lib.call("gngf_ext_sample_pixels", None, 4, 4, 3, 3.0, 0, None, 0, None, None, 1, None)


def test_every_entry_point_has_a_guarded_case_or_a_reason():
    from collision_handling_in_instantngp_amd import _lib
    import test_gpu_sampler as gs
    covered = set(gs.entry_points())
    names = set(_lib.EXT_SIGNATURES)
    assert covered <= names and set(WRITES_NOTHING) <= names
    missing = names - covered - set(WRITES_NOTHING)
    assert not missing, f"no guard-band case and no reason for: {sorted(missing)}"
    assert not covered & set(WRITES_NOTHING), sorted(covered & set(WRITES_NOTHING))
    assert all(isinstance(why, str) and why.strip() for why in WRITES_NOTHING.values())
    # the cases it counts are guard-band cases: the test that runs them checks the arena and that everything was written
    with open(os.path.join(ROOT, "tests", "test_gpu_sampler.py")) as f:
        body = f.read().split("def test_sample_pixels_guarded(")[1].split("\ndef ")[0]
    assert "arena.check()" in body and "unwritten" in body


def test_entry_points_listed_as_writing_nothing_take_no_writable_pointer():
    decl = header_functions()
    for name in WRITES_NOTHING:
        for param in decl[name]:
            assert "*" not in param or param.startswith("const "), f"{name} takes a writable pointer: {param}"
