"""The C-ABI of include/ramx_dist.h: every function it declares is in _lib.EXPORTS_DIST and exported by the library, its
parameter count equals the bound argtypes, and the record has the size the header promises (no compute calls)."""
import ctypes
import os
import re

import numpy as np

from repeatafterme_amd import _lib
from repeatafterme_amd.datamodel import COPY_DIST_DTYPE, COPY_DIST_FIELDS, DIST_MAX_COPIES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOT_FUNCTIONS = {"ramx_dist_cb"}


def _text():
    txt = open(os.path.join(ROOT, "include", "ramx_dist.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def _declared_arity():
    """-> {name: number of parameters}: the top-level commas of every parameter list, as tests/test_cabi.py counts them"""
    txt = _text()
    arity = {}
    for m in re.finditer(r"\b(ramx_[a-z0-9_]+)\s*\(", txt):
        depth, commas, at = 1, 0, m.end()
        while depth:
            ch = txt[at]
            depth += (ch == "(") - (ch == ")")
            commas += ch == "," and depth == 1
            at += 1
        inside = txt[m.end():at - 1].strip()
        arity[m.group(1)] = 0 if inside in ("", "void") else commas + 1
    for name in NOT_FUNCTIONS:
        arity.pop(name, None)
    return arity


def test_header_and_export_list_agree():
    assert set(_declared_arity()) == set(_lib.EXPORTS_DIST) and len(_lib.EXPORTS_DIST) == len(set(_lib.EXPORTS_DIST)) == 6
    assert not set(_lib.EXPORTS_DIST) & set(_lib.EXPORTS)
    assert '#include "ramx.h"' in open(os.path.join(ROOT, "include", "ramx_dist.h")).read()


def test_library_exports_every_declared_symbol():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in sorted(_declared_arity()):
        assert hasattr(lib, name), f"{name} declared in include/ramx_dist.h but not exported"


def test_every_prototype_has_the_headers_parameter_count():
    lib = _lib.lib()
    for name, n in _declared_arity().items():
        argtypes = getattr(lib, name).argtypes
        assert argtypes is not None and len(argtypes) == n, name
    assert lib.ramx_dist_kimura.restype is ctypes.c_double and lib.ramx_select_copies.restype is ctypes.c_int32


def test_record_sizes():
    assert ctypes.sizeof(_lib.CopyDistRec) == COPY_DIST_DTYPE.itemsize == 24
    assert tuple(k for k, _ in _lib.CopyDistRec._fields_) == COPY_DIST_FIELDS == COPY_DIST_DTYPE.names
    assert ctypes.sizeof(_lib.DistFamily) == 32
    m = re.search(r"#define\s+RAMX_DIST_MAX_COPIES\s+(\d+)", _text())
    assert m and int(m.group(1)) == DIST_MAX_COPIES == 2048
    # the library's own view of the layout: a record written field by field reads back through ramx_dist_kimura
    r = np.zeros(1, COPY_DIST_DTYPE)
    r["sites"], r["ts"], r["tv"] = 100, 0, 0
    assert _lib.lib().ramx_dist_kimura(r.ctypes.data) == 0.0
    r["tv"] = 50
    assert _lib.lib().ramx_dist_kimura(r.ctypes.data) == -1.0
