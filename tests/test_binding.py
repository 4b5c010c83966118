"""The ctypes binding is derived from include/picaso_hip.h: ``_lib.load()`` declares ``restype`` / ``argtypes`` for every
function of the header, so call sites pass plain Python values and a call that disagrees with the header raises in Python
instead of handing the library a truncated pointer or a register of garbage."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from picaso_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "picaso_amd")
I, L, S, D, P = ctypes.c_int, ctypes.c_long, ctypes.c_size_t, ctypes.c_double, ctypes.c_void_p


@pytest.fixture(scope="module")
def lib():
    from picaso_amd import build as b
    b.build(force=False)
    return _lib.load()


def test_every_declared_function_is_typed_from_the_header(lib):
    protos = _lib.declared_prototypes()
    assert sorted(protos) == _lib.declared_symbols() and len(protos) >= 110
    for name, (restype, argtypes) in protos.items():
        fn = getattr(lib, name)
        assert fn.argtypes is not None and list(fn.argtypes) == argtypes, name
        assert fn.restype is restype, name
    # written out by hand from the header
    assert protos["picaso_memcpy_h2d_2d"] == (I, [P, P, S, P, S, S, S])
    assert protos["picaso_stream"] == (P, [P])
    assert protos["picaso_version"] == (ctypes.c_char_p, [])
    assert protos["picaso_last_error"] == (ctypes.c_char_p, [P])
    assert protos["picaso_ctx_destroy"] == (None, [P])
    assert protos["picaso_host_setup_abi"] == (S, [])
    assert protos["picaso_thermal_nets_max_angles"] == (I, [])
    assert protos["picaso_mean_regrid_dev"] == (I, [P, L, I, P, I, P, P])                    # long nwno
    assert protos["picaso_reflected_1d_can_derive"] == (I, [I, L, I, I, P, P, D, I, I, D, I, I])    # long plane_pitch
    assert protos["picaso_axpby_dev"] == (I, [P, S, D, P, D, P, P])
    assert protos["picaso_host_setup_facets"] == (I, [P, I, L, P])
    assert protos["picaso_comm_group_max"] == (I, [I, P, P])                                 # a comment inside the parameter list
    assert protos["picaso_ck_from_xsec_dev"] == (I, [P, L, P, I, P, P, I, P, L, P, P])       # long long *: a pointer


# (where long and long long have one size, ctypes has one class for both: the later entry, long, is the one kept)
_C_PARAM = {I: "int", ctypes.c_longlong: "long long", L: "long", S: "size_t", D: "double", P: "void *"}
_C_RETURN = {I: "int", S: "size_t", P: "void *", ctypes.c_char_p: "const char *"}


def test_the_c_compiler_agrees_with_the_parser(tmp_path):
    """Independent of the regular expressions: a C file calls every function with extern variables of the C types the
    binding mapped its parameters to, and assigns the result to a variable of the mapped return type.  gcc rejects a
    wrong parameter count, a scalar classed as a pointer (or the reverse) and a narrowing or sign-changing scalar
    (-Wconversion, -Wsign-conversion, -Wint-conversion); -Wtraditional-conversion also rejects the widening ones (an
    ``int`` where the header says ``long`` or ``double``), which convert silently otherwise."""
    var = {ctype: "v_" + c.replace(" *", "_ptr").replace(" ", "_") for ctype, c in _C_PARAM.items()}
    lines = ["#include \"picaso_hip.h\""] + ["extern %s %s;" % (c, var[ctype]) for ctype, c in _C_PARAM.items()]
    for k, (name, (restype, argtypes)) in enumerate(sorted(_lib.declared_prototypes().items())):
        assert all(a in var for a in argtypes), name
        call = "%s(%s);" % (name, ", ".join(var[a] for a in argtypes))
        if restype is None:
            lines.append("void call_%d(void) { %s }" % (k, call))
        else:
            lines.append("%s r_%d; void call_%d(void) { r_%d = %s }" % (_C_RETURN[restype], k, k, k, call))
    src = tmp_path / "calls.c"
    src.write_text("\n".join(lines) + "\n")
    flags = ["-std=c99", "-fsyntax-only", "-Werror", "-Wconversion", "-Wsign-conversion", "-Wint-conversion",
             "-Wtraditional-conversion"]
    p = subprocess.run(["gcc"] + flags + ["-I", os.path.join(ROOT, "include"), str(src)], capture_output=True)
    assert p.returncode == 0, p.stderr.decode()[:4000]
    # the check has teeth: one int where the header says long, one argument short
    for good, bad in (("picaso_trapz_dev(v_void_ptr, v_long,", "picaso_trapz_dev(v_void_ptr, v_int,"),
                      ("picaso_sync(v_void_ptr);", "picaso_sync();")):
        text = src.read_text()
        assert good in text
        wrong = tmp_path / "wrong.c"
        wrong.write_text(text.replace(good, bad))
        p = subprocess.run(["gcc"] + flags + ["-I", os.path.join(ROOT, "include"), str(wrong)], capture_output=True)
        assert p.returncode != 0, bad


def test_an_unknown_type_is_an_error_at_load(monkeypatch, tmp_path):
    header = tmp_path / "picaso_hip.h"
    header.write_text("int picaso_fine(int a, const double *b);\nint picaso_odd(float scale);\n")
    monkeypatch.setattr(_lib, "HEADER", str(header))
    with pytest.raises(_lib.PicasoHipError, match="picaso_odd.*float scale"):
        _lib.declared_prototypes()
    header.write_text("short picaso_short(void);\n")
    with pytest.raises(_lib.PicasoHipError, match="picaso_short.*short"):
        _lib.declared_prototypes()


def _can_derive_args(wrap):
    u = np.full((5, 1), 0.5)
    i, l, d = (I, L, D) if wrap else (int, int, float)
    return (i(91), l(100000), i(5), i(1), _lib.ptr(u), _lib.ptr(u), d(1.0), i(3), i(0), d(2.0), i(0), i(0)), u


def test_wrong_calls_stop_in_python(lib):
    """picaso_reflected_1d_can_derive is host-only: no GPU needed."""
    fn = lib.picaso_reflected_1d_can_derive
    plain, keep = _can_derive_args(False)
    wrapped, keep2 = _can_derive_args(True)
    assert fn(*plain) == fn(*wrapped) == 1
    assert fn(*plain[:7], 1, *plain[8:]) == fn(*wrapped[:7], I(1), *wrapped[8:]) == 0        # another single_phase
    assert fn(np.int64(91), np.int32(100000), 5, True, *plain[4:6], 1, *plain[7:]) == 1   # numpy integers, bool, int for double
    with pytest.raises(TypeError):
        fn(*plain[:-1])
    with pytest.raises(ctypes.ArgumentError):
        fn(91.0, *plain[1:])
    with pytest.raises(ctypes.ArgumentError):
        fn(91, I(100000), *plain[2:])                    # a c_int for a long
    with pytest.raises(ctypes.ArgumentError):
        fn(*plain[:4], np.int64(keep.ctypes.data), *plain[5:])               # a numpy integer is no address: _lib.addr


def test_a_stale_library_is_reported_with_the_missing_names(lib, monkeypatch):
    protos = dict(_lib.declared_prototypes(), picaso_added_after_the_build=(I, [P]))
    monkeypatch.setattr(_lib, "declared_prototypes", lambda: protos)
    monkeypatch.setattr(_lib, "_lib", None)
    with pytest.raises(_lib.PicasoHipError, match="older sources.*picaso_added_after_the_build.*rebuild"):
        _lib.load()
    assert _lib._lib is None


def test_address_helpers():
    class Buffer:
        addr = 0x7f0012345678
    a = np.arange(8.0)
    assert _lib.addr(None) is None
    for x in (0x7f0012345678, np.int64(0x7f0012345678), np.uint64(0x7f0012345678), Buffer()):
        got = _lib.addr(x)
        assert type(got) is int and got == 0x7f0012345678
    assert type(_lib.addr(a)) is int and _lib.addr(a) == a.ctypes.data == a.__array_interface__["data"][0]
    table = _lib.ptr_array([a, None, Buffer()])
    assert isinstance(table, ctypes.Array) and len(table) == 3
    assert (table[0], table[1], table[2]) == (a.ctypes.data, None, 0x7f0012345678)            # None: NULL
    assert len(_lib.ptr_array([])) == 1 and _lib.ptr_array([])[0] is None
    P.from_param(table)                                                                        # a pointer parameter takes it
    assert _lib.ptr(None) is None
    for x in (a, Buffer(), 0x7f0012345678, np.int64(0x7f0012345678)):
        p = _lib.ptr(x)
        assert ctypes.cast(p, P).value == _lib.addr(x)
        P.from_param(p)
    assert _lib.ptr(a)[3] == 3.0


def _sources():
    for name in sorted(os.listdir(PKG)):
        if name.endswith(".py"):
            with open(os.path.join(PKG, name)) as fh:
                yield name, fh.read()


def test_the_binding_lives_in_one_module():
    defs = {"addr": [], "ptr_array": []}
    for name, text in _sources():
        if name != "_lib.py":
            assert not re.search(r"\.(argtypes|restype)\s*=[^=]", text), name
        assert not re.search(r"\b_c[idl]\b", text), "%s: a _ci / _cd / _cl alias" % name
        for helper in defs:
            if re.search(r"^\s*def _?%s\(" % helper, text, flags=re.M):
                defs[helper].append(name)
        assert not re.search(r"^\s*def (_dev|_table_ptrs|_addr|_ptr_array)\(", text, flags=re.M), name
    assert defs == {"addr": ["_lib.py"], "ptr_array": ["_lib.py"]}


@pytest.mark.gpu
def test_plain_values_round_trip_through_the_copies(lib):
    from picaso_amd.device import DeviceArray
    ctx = _lib.context()
    src, d, d2 = np.arange(8.0), DeviceArray((8,), ctx), DeviceArray((8,), ctx)
    assert type(d.addr) is int
    _lib.check(lib.picaso_memset(ctx, d.addr, 0xff, 64), ctx)
    back = np.zeros(8)
    _lib.check(lib.picaso_memcpy_d2h(ctx, _lib.ptr(back), d.addr, 64), ctx)
    assert back.tobytes() == b"\xff" * 64
    _lib.check(lib.picaso_memcpy_h2d(ctx, d.addr, _lib.ptr(src), 64), ctx)
    _lib.check(lib.picaso_memcpy_d2h(ctx, _lib.ptr(back), d.addr, 64), ctx)
    assert back.tobytes() == src.tobytes()
    # the form bench.py uses: c_void_p / c_size_t instances
    _lib.check(lib.picaso_memcpy_d2d(ctx, ctypes.c_void_p(d2.addr), ctypes.c_void_p(d.addr), ctypes.c_size_t(64)), ctx)
    assert d2.to_host().tobytes() == src.tobytes()
