"""the gzip-genome-batch-by-many-waves additions to the C ABI: three exports, their bindings, and no new status"""
import ctypes
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "metakssd_hip.h")
LIB = os.path.join(ROOT, "metakssd_amd", "lib", "libmetakssd_hip.so")
NEW = ("mk_sketch_batch_begin_gunzip", "mk_sketch_batch_gz_pieces", "mk_inflate_members_split")


def test_the_three_exports():
    lib = ctypes.CDLL(LIB)
    src = open(HEADER).read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert re.search(r"\bint %s\(" % name, src), "%s is not declared in the header" % name


def test_the_bindings():
    from metakssd_amd import capi
    assert len(capi.lib.mk_sketch_batch_begin_gunzip.argtypes) == 5
    assert len(capi.lib.mk_sketch_batch_gz_pieces.argtypes) == 3
    assert len(capi.lib.mk_inflate_members_split.argtypes) == 10
    assert "gunzip" in inspect.signature(capi.Engine.batch_begin_gz).parameters
    assert "split" in inspect.signature(capi.Inflate.members).parameters
    assert callable(capi.Engine.batch_gz_pieces)


def test_no_new_status_and_no_changed_struct():
    src = open(HEADER).read()
    vals = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (MK_INFL_[A-Z_]+) (\d+)", src)}
    assert vals == {"MK_INFL_MISSED": 9, "MK_INFL_CAPACITY": 10}
    from metakssd_amd import capi
    assert ctypes.sizeof(capi.GunzipOptsC) == 16 and ctypes.sizeof(capi.GunzipPiecesC) == 16 and ctypes.sizeof(capi.GzMemberResultC) == 16
    assert ctypes.sizeof(capi.GzMemberC) == 32 and ctypes.sizeof(capi.GzFileC) == 48
