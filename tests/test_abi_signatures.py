"""The ctypes signature table (cuda-winograd_amd/_abi.py) agrees with the prototypes in include/*.h: the same
functions, the same number of parameters, scalars of the same size, signedness and kind, pointer types where the
header has a pointer, and the two Structures field by field.  Reads the headers and the table only: no GPU and no
built library."""
import ctypes
import os
import re
import struct

import pytest

from conftest import ROOT

INCLUDE = os.path.join(ROOT, "include")

# C scalar -> (kind, bytes, signed) on the host that compiles the library (struct's native sizes, not the table's)
C_SCALARS = {
    "int": ("int", struct.calcsize("i"), True),
    "unsigned": ("int", struct.calcsize("I"), False),
    "unsigned int": ("int", struct.calcsize("I"), False),
    "long": ("int", struct.calcsize("l"), True),
    "size_t": ("int", struct.calcsize("N"), False),
    "uint64_t": ("int", 8, False),
    "unsigned long long": ("int", struct.calcsize("Q"), False),
    "float": ("float", 4, True),
    "double": ("float", 8, True),
    "char": ("char", 1, True),
}
# typedef -> (base type, extra pointer levels); struct typedef -> the Structure's name in the package
C_TYPEDEFS = {"wino_stream_t": ("void", 1)}
C_STRUCTS = {"wino_driver_result": "DriverResult", "wino_cpu_baseline_result": "CpuBaselineResult"}
TYPE_WORDS = {w for t in C_SCALARS for w in t.split()} | set(C_TYPEDEFS) | set(C_STRUCTS) | {"void"}


def _sources():
    for h in sorted(os.listdir(INCLUDE)):
        if h.endswith(".h"):
            yield h, re.sub(r"/\*.*?\*/", "", open(os.path.join(INCLUDE, h)).read(), flags=re.S)


def _c_type(decl: str, where: str):
    """'const float* in' / 'unsigned long long stamps[4]' / 'void' -> (base, pointer levels).  Raises ValueError on
    a base type this file does not know."""
    levels = decl.count("*") + len(re.findall(r"\[[^\]]*\]", decl))
    words = [w for w in re.sub(r"\[[^\]]*\]|\*", " ", decl).split() if w not in ("const", "struct")]
    if len(words) > 1 and words[-1] not in TYPE_WORDS:
        words.pop()                      # the parameter's (or field's) name
    base = " ".join(words)
    if base in C_TYPEDEFS:
        base, extra = C_TYPEDEFS[base]
        levels += extra
    if base not in C_SCALARS and base not in C_STRUCTS and base != "void":
        raise ValueError(f"{where}: unknown C type {base!r} in {decl.strip()!r}")
    return base, levels


def parse_prototypes(src: str, where: str = "<src>"):
    """{name: (return type, [parameter types])} of every function prototype in a comment-free header text."""
    protos = {}
    for m in re.finditer(r"^([A-Za-z_][\w\s\*]*?)\b(\w+)\s*\(([^;{]*)\)\s*;", src, flags=re.M):
        ret, name, params = m.group(1), m.group(2), m.group(3).strip()
        plist = [] if params in ("", "void") else [_c_type(p, f"{where}: {name}") for p in params.split(",")]
        protos[name] = (_c_type(ret, f"{where}: {name} (return)"), plist)
    return protos


def parse_structs(src: str, where: str = "<src>"):
    """{typedef name: [(field, C type)]} of every `typedef struct { ... } name;`."""
    out = {}
    for m in re.finditer(r"typedef\s+struct\s*\{(.*?)\}\s*(\w+)\s*;", src, flags=re.S):
        fields = []
        for decl in filter(None, (d.strip() for d in m.group(1).split(";"))):
            first, *more = decl.split(",")            # `int N, gpus`
            ctype = _c_type(first, f"{where}: {m.group(2)}")
            fields += [(n.strip(), ctype) for n in [first.split()[-1].lstrip("*")] + more]
        out[m.group(2)] = fields
    return out


def declared():
    protos, structs = {}, {}
    for h, src in _sources():
        protos.update(parse_prototypes(src, h))
        structs.update(parse_structs(src, h))
    return protos, structs


def _scalar(t):
    """(kind, bytes, signed) of a ctypes scalar, None for anything else."""
    code = getattr(t, "_type_", None)
    if not (isinstance(t, type) and issubclass(t, ctypes._SimpleCData)) or not isinstance(code, str):
        return None
    if code in "fdg":
        return "float", ctypes.sizeof(t), True
    if code in "bhilq" or code in "BHILQ":
        return "int", ctypes.sizeof(t), code.islower()
    return ("char", 1, True) if code == "c" else None


def _is_pointer(t):
    return isinstance(t, type) and (t in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(t, ctypes._Pointer))


def _describe(t):
    return getattr(t, "__name__", repr(t))


def _value_error(ctype, t, structs_py):
    """Why ctypes type `t` cannot carry the C type (base, levels); None when it can."""
    base, levels = ctype
    if levels == 0:
        if base == "void":
            return None if t is None else f"{_describe(t)} for void"
        if base in C_STRUCTS:
            return None if t is structs_py[C_STRUCTS[base]] else f"{_describe(t)} for struct {base}"
        return None if _scalar(t) == C_SCALARS[base] else f"{_describe(t)} for {base} {C_SCALARS[base]}"
    what = base + "*" * levels
    if not _is_pointer(t) or ctypes.sizeof(t) != ctypes.sizeof(ctypes.c_void_p):
        return f"{_describe(t)} for {what}: not a pointer type"
    if t is ctypes.c_char_p:
        return None if (base, levels) == ("char", 1) else f"c_char_p for {what}"
    if issubclass(t, ctypes._Pointer):
        inner = _value_error((base, levels - 1), t._type_, structs_py)
        return inner and f"POINTER({_describe(t._type_)}) for {what}: pointee is {inner}"
    # c_void_p carries any pointer: the binding's convention for tensors, workspaces and streams (callers pass
    # data_ptr() ints and None).  So a host out-parameter declared c_void_p instead of POINTER(<scalar>) passes here.
    return None


def mismatches(signatures, structs_py):
    """Every disagreement between the headers and `signatures` / the Structures `structs_py` {name: class}, as
    '<symbol>: ...' lines."""
    protos, structs_c = declared()
    bad = [f"{n}: declared in include/ but has no row" for n in sorted(set(protos) - set(signatures))]
    bad += [f"{n}: has a row but no prototype in include/" for n in sorted(set(signatures) - set(protos))]
    for name in sorted(set(protos) & set(signatures)):
        (ret, params), (restype, argtypes) = protos[name], signatures[name]
        err = _value_error(ret, restype, structs_py)
        if err is None and ret == ("char", 1) and restype is not ctypes.c_char_p:
            err = f"{_describe(restype)} for a string return: must be c_char_p"
        if err:
            bad.append(f"{name}: restype {err}")
        if len(params) != len(argtypes):
            bad.append(f"{name}: {len(argtypes)} argtypes for {len(params)} parameters")
            continue
        for k, (p, a) in enumerate(zip(params, argtypes)):
            err = _value_error(p, a, structs_py)
            if err:
                bad.append(f"{name}: argument {k}: {err}")
    for cname, pyname in C_STRUCTS.items():
        want, got = structs_c.get(cname), structs_py[pyname]._fields_
        if want is None:
            bad.append(f"{pyname}: no typedef struct {cname} in include/")
        elif [f for f, _ in want] != [f for f, _ in got]:
            bad.append(f"{pyname}: fields {[f for f, _ in got]}, {cname} has {[f for f, _ in want]}")
        else:
            bad += [f"{pyname}.{f}: {e}" for (f, c), (_, t) in zip(want, got)
                    for e in [_value_error(c, t, structs_py)] if e]
    return bad


@pytest.fixture
def structs_py(pkg):
    return {"DriverResult": pkg.DriverResult, "CpuBaselineResult": pkg.CpuBaselineResult}


def test_signature_table_matches_the_headers(pkg, structs_py):
    protos, structs_c = declared()
    assert set(protos) == set(pkg.SIGNATURES), set(protos) ^ set(pkg.SIGNATURES)
    assert pkg.ABI_SYMBOLS == list(pkg.SIGNATURES)
    assert set(C_STRUCTS) == set(structs_c)
    bad = mismatches(pkg.SIGNATURES, structs_py)
    assert not bad, "\n".join(bad)


def test_headers_use_every_scalar_the_check_covers():
    """The rules above are exercised: each scalar appears as a parameter or pointee, and each return kind occurs."""
    protos, _ = declared()
    used = {base for _, params in protos.values() for base, _ in params}
    assert {"int", "unsigned", "long", "size_t", "uint64_t", "unsigned long long", "float", "double"} <= used
    returns = {ret for ret, _ in protos.values()}
    assert {("int", 0), ("long", 0), ("size_t", 0), ("uint64_t", 0), ("float", 0), ("char", 1), ("float", 1)} <= returns


def test_parser_reads_every_parameter_form():
    protos = parse_prototypes("int f(const float* a, void** b, wino_stream_t s, wino_stream_t* t,\n"
                              "      unsigned long long st[4], long n, unsigned v, wino_driver_result* r);\n"
                              "const char* g(void);\nuint64_t h(void);\n")
    assert protos["f"] == (("int", 0), [("float", 1), ("void", 2), ("void", 1), ("void", 2), ("unsigned long long", 1),
                                        ("long", 0), ("unsigned", 0), ("wino_driver_result", 1)])
    assert protos["g"] == (("char", 1), []) and protos["h"] == (("uint64_t", 0), [])


@pytest.mark.parametrize("proto", ["int f(half x);", "int f(const short* p, int n);", "__int128 f(void);",
                                   "int f(struct foo* p);"])
def test_parser_fails_loudly_on_an_unknown_type(proto):
    with pytest.raises(ValueError, match="unknown C type"):
        parse_prototypes(proto)
    with pytest.raises(ValueError, match="unknown C type"):
        parse_structs("typedef struct { double us; half x; } s_t;")


def test_the_check_catches_wrong_rows(pkg, structs_py):
    """A wrong declaration is memory corruption on the GPU machine, not a failure anywhere else: each kind of mistake
    must be reported here, under the symbol's name."""
    c_int, c_long, c_size_t, c_void_p = ctypes.c_int, ctypes.c_long, ctypes.c_size_t, ctypes.c_void_p

    def broken(name, restype=..., argtypes=None):
        sig = dict(pkg.SIGNATURES)
        r, a = sig[name]
        sig[name] = (r if restype is ... else restype, list(a) if argtypes is None else argtypes(list(a)))
        return [b for b in mismatches(sig, structs_py)]

    def only(bad, symbol):
        return bad and all(b.startswith(symbol + ":") or b.startswith(symbol + ".") for b in bad)

    assert only(broken("wino_conv1x1_prepare", argtypes=lambda a: [c_int] + a[1:]), "wino_conv1x1_prepare")   # long M
    assert only(broken("wino_head_workspace_bytes", restype=c_int), "wino_head_workspace_bytes")   # the ctypes default
    assert only(broken("wino_conv3x3_plan", argtypes=lambda a: a[:5] + a[6:]), "wino_conv3x3_plan")   # one int too few
    assert only(broken("wino_malloc", argtypes=lambda a: [c_size_t, c_size_t]), "wino_malloc")     # an int for a void**
    assert only(broken("wino_conv3x3_plan", argtypes=lambda a: a[:8] + [ctypes.POINTER(c_int)] + a[9:]),
                "wino_conv3x3_plan")                                                                 # long* tail_iters
    assert only(broken("wino_last_error_string", restype=c_void_p), "wino_last_error_string")
    assert only(broken("wino_driver_last_output", restype=c_int), "wino_driver_last_output")       # const float* return
    assert only(broken("wino_driver_pack_times", argtypes=lambda a: [ctypes.c_int64, a[1]]), "wino_driver_pack_times")
    assert only(broken("wino_debug_conv1x1_models", argtypes=lambda a: a[:4] + [ctypes.POINTER(ctypes.c_float)] * 2),
                "wino_debug_conv1x1_models")
    sig = dict(pkg.SIGNATURES)
    del sig["wino_abi_version"]
    assert only(mismatches(sig, structs_py), "wino_abi_version")

    class Short(ctypes.Structure):                    # DriverResult without its last field
        _fields_ = pkg.DriverResult._fields_[:-1]

    class Narrow(ctypes.Structure):                   # error_cnt as an int
        _fields_ = [(f, c_int if f == "error_cnt" else t) for f, t in pkg.DriverResult._fields_]

    for cls in (Short, Narrow):
        bad = mismatches(pkg.SIGNATURES, dict(structs_py, DriverResult=cls))
        # (the rows that point at the real DriverResult are reported too: the class is part of the signature)
        assert any(b.startswith("DriverResult") for b in bad), bad
