"""the member-concatenation additions to the gunzip C ABI: exports, the flag, the status and its text, and struct
layouts that kept their sizes"""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "metakssd_hip.h")
LIB = os.path.join(ROOT, "metakssd_amd", "lib", "libmetakssd_hip.so")


def test_exports():
    lib = ctypes.CDLL(LIB)
    for name in ("mk_inflate_stream_members", "mk_gunzip_status_text"):
        assert hasattr(lib, name), name


def test_flag_status_and_text():
    src = open(HEADER).read()
    assert re.search(r"#define MK_GUNZIP_MEMBERS 1u\b", src)
    assert re.search(r"#define MK_INFL_BAD_MEMBER \(MK_INFL_CAPACITY \+ 1\)", src) and re.search(r"#define MK_INFL_CAPACITY 10\b", src)
    assert re.search(r"#define MK_GUNZIP_PIECE_MEMBER \(\(uint64_t\)1 << 63\)", src)
    from metakssd_amd import capi
    assert (capi.MK_GUNZIP_MEMBERS, capi.MK_INFL_BAD_MEMBER, capi.MK_GUNZIP_PIECE_MEMBER) == (1, 11, 1 << 63)
    text = capi.lib.mk_gunzip_status_text(11)
    assert text and text != b"unknown status"
    assert all(capi.lib.mk_gunzip_status_text(s) == capi.lib.mk_inflate_status_text(s) for s in list(range(11)) + [12, -1])
    assert text not in {capi.lib.mk_inflate_status_text(s) for s in range(11)}


def test_layouts_kept_their_sizes():
    from metakssd_amd import capi
    assert [n for n, _ in capi.GunzipOptsC._fields_] == ["span_bytes", "ratio", "batch_spans", "flags"]
    assert capi.GunzipStatsC._fields_[-1] == ("members", ctypes.c_uint32)
    assert (ctypes.sizeof(capi.GunzipOptsC), ctypes.sizeof(capi.GunzipPieceC), ctypes.sizeof(capi.GunzipPiecesC), ctypes.sizeof(capi.GunzipStatsC)) == (16, 16, 16, 104)
    assert capi.GunzipOptsC.flags.offset == 12 and capi.GunzipStatsC.members.offset == 100
