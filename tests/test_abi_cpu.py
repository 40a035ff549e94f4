"""CPU: the C-ABI shared library loads without a GPU, exports every symbol include/ada_hip.h declares, the ctypes prototype table agrees with the
header's declarations argument by argument, and the ctypes mirrors of the argument structs have exactly the C layout (checked by compiling the
header with gcc)."""
import ctypes
import os
import re
import subprocess

import pytest

import hip_ext
from hip_ext import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ada_hip.h")


def _header_text():
    src = open(HEADER).read()
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", src, flags=re.S))


def _declared_functions():
    return sorted(set(re.findall(r"\b(ada_[a-z0-9_]+)\s*\(", _header_text())))


def _declarations():
    """name -> (return type, [(base type, is pointer)]) of every ``<type> ada_*(...);`` in the header, in its order."""
    out = {}
    for ret, name, args in re.findall(r"(const\s+char\s*\*|\bint|\bvoid)\s*(ada_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", _header_text()):
        params = []
        for a in (() if args.strip() == "void" else args.split(",")):
            m = re.fullmatch(r"\s*(?:const\s+)?(\w+)\s*(\*?)\s*\w+\s*", a)
            assert m, f"{name}: cannot read the parameter {a!r}"
            params.append((m.group(1), bool(m.group(2))))
        assert name not in out, name
        out[name] = (" ".join(ret.split()), params)
    return out


_SCALARS = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "int": ctypes.c_int, "uint32_t": ctypes.c_uint32, "uint8_t": ctypes.c_uint8,
            "float": ctypes.c_float, "double": ctypes.c_double}
_STRUCTS = {"ada_igemm_args": hip_ext.IgemmArgs, "ada_layernorm_args": hip_ext.LayerNormArgs}
_RETURNS = {"int": ctypes.c_int, "void": None, "const char*": ctypes.c_char_p, "const char *": ctypes.c_char_p}


def _arg_matches(base, is_pointer, ctype):
    if not is_pointer:
        return ctype is _SCALARS[base]
    if base in _STRUCTS:
        return ctype is ctypes.POINTER(_STRUCTS[base])
    return ctype is ctypes.c_void_p or (base in _SCALARS and ctype is ctypes.POINTER(_SCALARS[base]))


def _prototype_mismatches(prototypes, declarations):
    """Every disagreement between a prototype table and the header's declarations, as text."""
    bad = [f"{n}: declared, no prototype" for n in declarations if n not in prototypes] + [f"{n}: prototype, not declared" for n in prototypes if n not in declarations]
    for name, (ret, params) in declarations.items():
        if name not in prototypes:
            continue
        restype, argtypes = prototypes[name]
        if restype is not _RETURNS[ret]:
            bad.append(f"{name}: returns {ret}, prototype says {restype}")
        if len(argtypes) != len(params):
            bad.append(f"{name}: {len(params)} parameters, prototype has {len(argtypes)}")
            continue
        bad += [f"{name}: parameter {i} is {base}{'*' if ptr else ''}, prototype says {t.__name__}"
                for i, ((base, ptr), t) in enumerate(zip(params, argtypes)) if not _arg_matches(base, ptr, t)]
    return bad


def test_library_loads_and_exports_every_declared_symbol():
    lib = hip_ext.load()
    names = _declared_functions()
    assert set(names) == set(hip_ext.EXPORTS), (names, hip_ext.EXPORTS)
    for n in names:
        assert hasattr(lib, n), f"{n} declared in ada_hip.h but not exported"
    assert lib.ada_abi_version() == hip_ext.ABI_VERSION
    assert lib.ada_operand_dtype() in (hip_ext.DT_F16, hip_ext.DT_BF16)
    assert lib.ada_last_error() is not None


def test_prototypes_match_header():
    decl = _declarations()
    assert len(decl) == len(hip_ext.EXPORTS)
    assert set(decl) == set(hip_ext.EXPORTS) == set(_declared_functions())       # the declaration parse finds every name the looser one finds
    assert list(decl) == list(hip_ext.EXPORTS), "PROTOTYPES is kept in the header's order"
    assert hip_ext.EXPORTS == tuple(hip_ext.PROTOTYPES)
    assert _prototype_mismatches(hip_ext.PROTOTYPES, decl) == []
    lib = hip_ext.load()
    for name, (restype, argtypes) in hip_ext.PROTOTYPES.items():      # load() applied the table
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name


def test_prototype_comparator_reports_a_wrong_type_and_a_dropped_argument():
    decl = _declarations()
    table = {k: (r, list(a)) for k, (r, a) in hip_ext.PROTOTYPES.items()}      # a copy: the live table is never altered
    args = table["ada_range_map_fwd"][1]
    i = args.index(ctypes.c_float)
    args[i] = ctypes.c_double
    table["ada_mask_stats_fwd"][1].pop()
    table["ada_debug_last_tile"] = (None, [])
    bad = _prototype_mismatches(table, decl)
    assert len(bad) == 3, bad
    assert any(b.startswith(f"ada_range_map_fwd: parameter {i} is float") and "c_double" in b for b in bad), bad
    assert any(b.startswith("ada_mask_stats_fwd: 8 parameters, prototype has 7") for b in bad), bad
    assert any(b.startswith("ada_debug_last_tile: returns int") for b in bad), bad
    del table["ada_selftest"]
    assert "ada_selftest: declared, no prototype" in _prototype_mismatches(table, decl)
    assert _prototype_mismatches(hip_ext.PROTOTYPES, decl) == []


def test_bf16_variant_library_exports_the_same_abi():
    path = hip_ext.library_path(bf16=True)
    if not os.path.exists(path):
        pytest.skip("bf16 measurement variant not built")
    lib = ctypes.CDLL(path)
    for n in hip_ext.EXPORTS:
        assert hasattr(lib, n)
    lib.ada_operand_dtype.restype = ctypes.c_int
    assert lib.ada_operand_dtype() == hip_ext.DT_BF16


@pytest.mark.parametrize("struct,cname", [(hip_ext.IgemmArgs, "ada_igemm_args"), (hip_ext.LayerNormArgs, "ada_layernorm_args")], ids=["igemm", "layernorm"])
def test_args_struct_layout_matches_c(tmp_path, struct, cname):
    names = [f[0] for f in struct._fields_]
    cnames = ["in" if f == "in_" else f for f in names]
    prog = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){", f'printf("%zu\\n", sizeof({cname}));']
    prog += [f'printf("%zu\\n", offsetof({cname}, {f}));' for f in cnames]
    prog += ["return 0;}"]
    c = tmp_path / "layout.c"
    c.write_text("\n".join(prog))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-o", str(exe), str(c)])
    vals = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert vals[0] == ctypes.sizeof(struct)
    for f, off in zip(names, vals[1:]):
        assert getattr(struct, f).offset == off, f


def test_constants_match_header():
    src = open(HEADER).read()
    consts = {m.group(1): int(m.group(2), 0) for m in re.finditer(r"#define\s+(ADA_[A-Z0-9_]+)\s+\(?(-?(?:0x)?[0-9A-Fa-f]+)\)?\s", src)}
    valued = re.findall(r"^[ \t]*#define[ \t]+(ADA_\w+)[ \t]+[^\s/]", src, flags=re.M)       # every #define ADA_* that has a value (not the include guard)
    assert sorted(valued) == sorted(consts) and consts["ADA_ELAUNCH"] == -3 and consts["ADA_EP_RELU_F32"] == 0x80
    for name, val in consts.items():
        assert getattr(hip_ext, name[4:]) == val, name


def test_missing_library_fails_loudly(tmp_path, monkeypatch):
    monkeypatch.setattr(_abi, "_lib", None)
    with pytest.raises(hip_ext.HipExtError, match="no CPU fallback"):
        hip_ext.load(str(tmp_path / "nope.so"))
    hip_ext.load()  # restore
