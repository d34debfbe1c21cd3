"""mk_sketch_push_gzip_q, the -n / -Q reader's entry point of the many-waves-a-stream gunzip, in the C ABI: the
header's declaration, the library's export, the binding's argument list and the Engine method"""
import ctypes
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "metakssd_hip.h")
LIB = os.path.join(ROOT, "metakssd_amd", "lib", "libmetakssd_hip.so")


def test_header_declares_it():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+mk_sketch_push_gzip_q\s*\(([^)]*)\)\s*;", src)
    assert m, "include/metakssd_hip.h does not declare mk_sketch_push_gzip_q"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["mk_engine *e", "int fd", "size_t size", "const mk_gunzip_opts *opts", "int32_t qmin", "uint64_t first_ordinal",
                    "mk_gunzip_stats *st"]


def test_library_exports_it():
    lib = ctypes.CDLL(LIB)
    assert hasattr(lib, "mk_sketch_push_gzip_q")
    assert hasattr(lib, "mk_sketch_push_gzip")  # the -A entry point stays


def test_binding():
    from metakssd_amd import capi
    fn = capi.lib.mk_sketch_push_gzip_q
    assert len(fn.argtypes) == 7 and fn.restype is ctypes.c_int
    assert fn.argtypes[4] is ctypes.c_int32 and fn.argtypes[5] is ctypes.c_uint64
    assert len(capi.lib.mk_sketch_push_gzip.argtypes) == 6
    sig = inspect.signature(capi.Engine.push_gzip_q)
    assert list(sig.parameters) == ["self", "path", "qmin", "span_bytes", "ratio", "batch_spans", "first_ordinal", "members"]
    assert [p.default for p in list(sig.parameters.values())[2:]] == [0, 0, 0, 0, 0, False]
