"""CPU tests of the Python binding's entry table (no GPU): fa_mi355x.C_ENTRIES
against the declarations of include/fa_mi355x.h, the one independent statement
of the C lists the ctypes argtypes have; that load_library() gives every
function exactly the table's types; and that no resolved entry outlives the
library it came from.  The first needs no built library."""
import ctypes
import re

import capi_checks as cc
import fa_mi355x as fa

# header type -> ctypes type; every other pointer is a c_void_p
SCALARS = {"int": ctypes.c_int, "long long": ctypes.c_longlong, "unsigned long long": ctypes.c_ulonglong}
STRUCTS = {"fa_config_info_t*": ctypes.POINTER(fa._ConfigInfo),
           "fa_kernel_attrs_t*": ctypes.POINTER(fa._KernelAttrs)}
# the parameter types the header uses: the scalars, the two structures, `void`
# (no parameters) and these pointers
POINTERS = {"const void*", "void*", "const int*", "const float*", "float*", "hipStream_t"}


def _ctype(decl, is_return):
    """The ctypes type of a parameter declaration (`const int* kv_lens`) or of
    a return type (`const char*`)."""
    ty = decl if is_return else re.sub(r"\b[A-Za-z_]\w*$", "", decl)  # the parameter's name
    ty = re.sub(r"\s*\*\s*", "*", " ".join(ty.split()))
    if is_return and ty == "const char*":
        return ctypes.c_char_p
    if ty in SCALARS:
        return SCALARS[ty]
    if ty in STRUCTS:
        return STRUCTS[ty]
    assert ty in POINTERS, f"a type this test has no mapping for: {ty!r} in {decl!r}"
    return ctypes.c_void_p


def _declarations():
    """[(name, restype, argtypes)] of every function fa_mi355x.h declares:
    test_capi.py's regex with groups for the return type and the parameters."""
    found = re.findall(r"^([A-Za-z_][\w \*]*?)\b([a-z_][a-z0-9_]*)\s*\(([^;{]*)\)\s*;",
                       cc.header_text("fa_mi355x.h"), re.M)
    out = []
    for ret, name, params in found:
        params = [p.strip() for p in params.split(",")]
        if params == ["void"] or params == [""]:
            params = []
        out.append((name, _ctype(ret.strip(), True), [_ctype(p, False) for p in params]))
    return out


def test_table_matches_the_header():
    decls = _declarations()
    names = [name for name, _, _ in decls]
    assert len(names) == len(set(names)), sorted(n for n in names if names.count(n) > 1)
    assert len(fa.EXPORTED_SYMBOLS) == len(set(fa.EXPORTED_SYMBOLS)) == len(fa.C_ENTRIES)
    assert set(names) == set(fa.C_ENTRIES) == set(fa.EXPORTED_SYMBOLS), \
        sorted(set(names) ^ set(fa.C_ENTRIES))
    assert len(names) == 132
    wrong = [(name, restype, argtypes, fa.C_ENTRIES[name]) for name, restype, argtypes in decls
             if fa.C_ENTRIES[name] != (restype, argtypes)]
    assert not wrong, wrong[:3]


def test_every_row_is_its_own_list():
    """A row is never another row's list: changing one function's argtypes
    cannot change another's."""
    lists = [id(argtypes) for _, argtypes in fa.C_ENTRIES.values()]
    assert len(lists) == len(set(lists))


def test_load_library_sets_the_tables_types():
    lib = fa.load_library()
    for name, (restype, argtypes) in fa.C_ENTRIES.items():
        fn = getattr(lib, name)
        assert fn.restype is restype, name
        assert list(fn.argtypes) == argtypes, name


def test_entries_follow_the_library(monkeypatch):
    """After the tools' swap idiom (fa._lib = None, load_library(); or fa._lib =
    another library) every entry is resolved in the current library."""
    names = [fa._entry_name("fa_decode", "_win", True, True, False),
             fa._entry_name("fa_prefill", "", False, False, True)]
    assert names == ["fa_decode_win_paged_kv8_f16", "fa_prefill_bf16"]
    first = fa.load_library()
    before = [fa._entry(n) for n in names]
    assert all(f is getattr(first, n) for f, n in zip(before, names))
    monkeypatch.setattr(fa, "_lib", None)
    second = fa.load_library()
    assert second is not first and fa._lib is second
    after = [fa._entry(n) for n in names]
    assert all(f is getattr(second, n) for f, n in zip(after, names))
    assert not any(f is g for f, g in zip(before, after))
    # a direct assignment, as tools/ab.py does it
    monkeypatch.setattr(fa, "_lib", first)
    assert all(fa._entry(n) is f for n, f in zip(names, before))
